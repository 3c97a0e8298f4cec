"""The caller's memory under guard, outside the resize entry points: impgpu_batch_filters and every operator that works in
place on a wrapped window (pointwise filters, the HSV stages, ASCII, BlendWithPaper, Watermark, the Gaussian forms no
one-pass kernel takes) or reads a wrapped window and writes a fresh frame (flip, rotate, crop, gray promotion, the one-pass
Gaussians), alone and through impgpu_batch_run_ops.

Each frame is a window inside a parent of random bytes (window_guard) in an alignment class -- the property the launchers
choose their kernels by: the 16-byte and 12-byte pixel programs against the scalar one, k_blend_over's dword branch,
k_rotate_bgr's dword tiles, k_copy<4> / k_copy_run, the matrix-unit Gaussian's unaligned source rows.  After the call the
pixels equal the CPU oracle's exactly (vignette: within one, as test_gpu_filters has it) and every byte of the parent
outside the windows equals the copy from before; where the operator writes a fresh frame, the windows do too.

Shapes are (width, height)."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from window_guard import KINDS, GuardedParent, WindowLayout, describe, layout_for, locate

pytestmark = pytest.mark.gpu

INVALID_ARGS = 50
CLASSES_OF = {1: ("a16", "a4", "a1"), 3: ("a16", "a4", "a1"), 4: ("a16", "a4")}      # BGRA off the 4-byte grid is refused

# one program per kernel template: a single table (LUT_ONLY), HSV + tables (the stage loop), stages that need (x, y)
PROGRAMS = {"table": ["gamma=1.7"], "hsv+tables": ["gotham=1", "gamma=1.7"], "xy": ["scanline=0.6,0.4,3,2", "contrast=1.2"]}
VIGNETTE = ["vignette=0.8,0.6"]
VIGNETTE_SIZE = (160, 120)                     # test_vignette_within_one's frame

# ---- the sizes (the host test of the helper checks that every kind of layout is in its class at each of them)
VEC, ODD = (36, 32), (35, 31)                  # 1152 pixels = 288 groups: a partial second workgroup; 1085 pixels: npix % 4 != 0
BIG, BIG_COUNT = (500, 524), 65                # 17.03 M pixels >= 16 << 20; 65500 groups a frame, no multiple of 1024
SMALL = [(53, 37), (7, 5)]
ASCII_SIZE = (72, 30)
WM_BASE, WM_OVERLAY, WM_HUGE = (120, 90), (40, 24), (130, 100)
BLUR_SIZES = [(67, 45), (131, 70)]
THIN = [(40, 1), (1, 40)]
ROTATE_SIZES = [(96, 64), (130, 70), (31, 31)]
ODD_COLUMN = (65, 64)                          # rotate=270: full tiles whose first source column is 33 or 1, 99 or 3 bytes in
ONE_PASS_SIZES = [(67, 45), (131, 70), (200, 9)]
BATCH_SIZES = [(53, 37), (67, 45), (96, 64), (131, 70)]
ALL_SIZES = sorted(set([VEC, ODD, VIGNETTE_SIZE, ASCII_SIZE, WM_BASE, ODD_COLUMN] + SMALL + BLUR_SIZES + THIN + ROTATE_SIZES
                       + ONE_PASS_SIZES + BATCH_SIZES))
CROP = "31px,17px,13px,9px"

_REF = {}


def ref(key, make):
    """The oracle's answer for `key`, computed once for the session and never written to."""
    if key not in _REF:
        out = make()
        if isinstance(out, np.ndarray):
            out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def frame(w, h, c, seed):
    return ref(("noise", w, h, c, seed), lambda: noise_image(h, w, c, 9100 + seed))


def chain(arr, filters):
    cur = arr
    for f in filters:
        rc, cur = orc.filter(cur, f)
        assert rc == 0, f
    return cur


def chained(tag, arr, filters):
    return ref(("chain", tag, arr.shape, tuple(filters)), lambda: chain(arr, filters))


def within_one(got, want, where):
    d = np.abs(got.astype(int) - want.astype(int))
    assert d.max() <= 1, where
    assert (d > 0).mean() < 1e-3, where


def guarded(gpu, kind, arr, seed=0):
    """arr (h, w, c) as the only window of a parent of `kind`, wrapped -> (parent, Image)."""
    h, w, c = arr.shape
    g = GuardedParent(layout_for(kind, w, h, c), [arr], seed)
    return g, g.wrap(gpu, w, h, c)


def on_window(g, im):
    """Does the handle still stand on the caller's window?  (A fresh frame is pool memory, never inside the parent.)"""
    return im.device_ptr == g.ptr()


def in_place(gpu, g, im, want, where, approx=False):
    """The operator worked on the window: the handle still stands on it, it holds `want`, nothing else changed."""
    rep = g.report(gpu)
    same = on_window(g, im)
    im.release()
    assert same, where
    got = rep.windows[0].reshape(want.shape)
    if approx:
        within_one(got, want, where)
    else:
        assert np.array_equal(got, want), where
    assert rep.intact, (where, describe(rep))


def fresh_frame(gpu, g, im, want, where):
    """The operator wrote a frame of its own: it holds `want`, the whole parent is as before."""
    got = im.numpy()
    rep = g.report(gpu, fresh=True)
    im.release()
    assert got.shape == want.shape and np.array_equal(got, want), where
    assert rep.intact, (where, describe(rep))


def refused(gpu, g, im, rc, where):
    rep = g.report(gpu, fresh=True)
    im.release()
    assert rc == INVALID_ARGS, (where, rc)
    assert rep.intact, (where, describe(rep))


def test_the_guard_reads_the_device(gpu):
    """The report compares what the device holds, not the host copy with itself: a byte flipped there (by torch, one past a
    row's end and inside a window) is found where it is.  That a planted byte is named rightly in every place is
    test_window_guard.py's, on the host."""
    import torch

    w, h, c = 21, 9, 3
    lay = layout_for("a4", w, h, c, 3)
    g = GuardedParent(lay, [frame(w, h, c, i) for i in range(3)])
    assert g.report(gpu).intact and g.report(gpu, fresh=True).intact
    outside, inside = lay.offset + lay.stride + 2 * lay.step + lay.row_bytes, lay.offset + 2 * lay.stride + 4 * lay.step + 5
    g.dev[inside] ^= 0x01
    torch.cuda.synchronize()
    rep = g.report(gpu)
    assert rep.intact and rep.windows[2, 4, 5] == g.before[inside] ^ 0x01
    rep = g.report(gpu, fresh=True)
    assert not rep.intact and rep.touched == [(inside, inside - lay.offset)] and locate(lay, inside) == (2, 4, 5)
    g.dev[outside] ^= 0x40
    torch.cuda.synchronize()
    rep = g.report(gpu)
    assert not rep.intact and rep.touched == [(outside, outside - lay.offset)] and locate(lay, outside) == (1, 2, lay.row_bytes)
    assert "frame 1 row 2 col-byte %d" % lay.row_bytes in describe(rep)


# ================================================================= a. impgpu_batch_filters
# (kind, size, channel counts): contiguous on the 16-byte grid -- k_pixel_program_v4<4 | 3>; a padded pitch -- scalar; a
# pixel count that is no multiple of 4 -- scalar; the start on the 4-byte grid -- BGRA scalar, BGR still 12-byte groups; the
# frame stride on the 4-byte grid -- the same split; everything odd -- BGR scalar
BATCH_LAYOUTS = [("contig", VEC, (3, 4)), ("a16", VEC, (3, 4)), ("contig", ODD, (3, 4)), ("contig-a4", VEC, (3, 4)),
                 ("contig-s4", VEC, (3, 4)), ("a1", VEC, (3,))]


def batch_filters_case(gpu, kind, size, c, frames, filters, count, want, where, approx=False):
    w, h = size
    lay = layout_for(kind, w, h, c, count)
    g = GuardedParent(lay, frames, seed=c)
    rc = gpu.batch_filters(g.ptr(), lay.stride, w, h, c, lay.step, count, filters)
    rep = g.report(gpu)
    assert rc == 0, (where, rc)
    got = rep.windows.reshape(count, h, w, c)
    for i in range(len(frames), count):                                # the sources repeat: so must the answers
        assert np.array_equal(got[i], got[i % len(frames)]), (where, "frame", i)
    for i in range(len(frames)):
        if approx:
            within_one(got[i], want[i], (where, i))
        else:
            assert np.array_equal(got[i], want[i]), (where, "oracle", i)
    assert rep.intact, (where, describe(rep))


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_batch_filters_under_guard(gpu, program, c):
    for kind, (w, h), cs in BATCH_LAYOUTS:
        if c not in cs:
            continue
        frames = [frame(w, h, c, i) for i in range(3)]
        want = [chained(i, f, PROGRAMS[program]) for i, f in enumerate(frames)]
        batch_filters_case(gpu, kind, (w, h), c, frames, PROGRAMS[program], 3, want, (program, c, kind, w, h))


@pytest.mark.parametrize("c", [3, 4])
def test_batch_filters_vignette_under_guard(gpu, c):
    w, h = VIGNETTE_SIZE
    frames = [ref(("smooth", w, h, c, i), lambda: smooth_image(h, w, c, i)) for i in range(3)]
    want = [chained(("smooth", i), f, VIGNETTE) for i, f in enumerate(frames)]
    for kind in ("contig", "a16", "contig-a4", "contig-s4") + (("a1",) if c == 3 else ()):
        batch_filters_case(gpu, kind, (w, h), c, frames, VIGNETTE, 3, want, ("vignette", c, kind), approx=True)


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("program", ["table", "xy"])
def test_batch_filters_four_groups_per_thread(gpu, program, c):
    """65 frames of 500 x 524 are 17.03 M pixels, past the 16 << 20 from which a thread carries four groups; a frame's 65500
    groups are 63 whole workgroups of 1024 and one of 988.  The sources repeat with period 3."""
    w, h = BIG
    assert w * h * BIG_COUNT >= 16 << 20 and (w * h // 4) % 1024
    frames = [frame(w, h, c, 20 + i) for i in range(3)]
    want = [chained(20 + i, f, PROGRAMS[program]) for i, f in enumerate(frames)]
    batch_filters_case(gpu, "contig", BIG, c, frames, PROGRAMS[program], BIG_COUNT, want, (program, c, "big"))


def test_batch_filters_refuses_bgra_off_the_grid(gpu):
    """An odd start, an odd pitch or an odd frame stride alone: IMP_ERROR_INVALID_ARGS, and no byte changes."""
    w, h = VEC
    frames = [frame(w, h, 4, i) for i in range(3)]
    odd_pitch = WindowLayout(w * 4, h, 3, "a1", start="a16", stride_cls="a16")
    odd_stride = WindowLayout(w * 4, h, 3, "a16", stride_cls="a1")
    for lay, shift in ((layout_for("a1", w, h, 4, 3), 0), (layout_for("a16", w, h, 4, 3), 1), (odd_pitch, 0), (odd_stride, 0)):
        g = GuardedParent(lay, frames)
        rc = gpu.batch_filters(g.ptr() + shift, lay.stride, w, h, 4, lay.step, 3, PROGRAMS["table"])
        rep = g.report(gpu, fresh=True)
        assert rc == INVALID_ARGS, (lay.offset + shift, lay.step, lay.stride, rc)
        assert rep.intact, describe(rep)


# ================================================================= b. in place on a wrapped window
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("program", sorted(PROGRAMS))
def test_filter_in_place(gpu, program, c):
    """impgpu_filter, one call per filter.  The padded classes take the scalar kernel; the contiguous 36 x 32 window the
    vector kernels with a frame stride of 0 (BGRA on the 4-byte grid: scalar)."""
    cases = [(kind, size) for kind in CLASSES_OF[c] for size in SMALL] + [("contig", VEC), ("contig-a4", VEC), ("contig", ODD)]
    for kind, (w, h) in cases:
        arr = frame(w, h, c, 0)
        g, im = guarded(gpu, kind, arr)
        for f in PROGRAMS[program]:
            assert im.filter(f) == 0, (f, kind)
        in_place(gpu, g, im, chained(0, arr, PROGRAMS[program]), (program, c, kind, w, h))


@pytest.mark.parametrize("c", [3, 4])
def test_vignette_in_place(gpu, c):
    w, h = VIGNETTE_SIZE
    arr = ref(("smooth", w, h, c, 0), lambda: smooth_image(h, w, c, 0))
    for kind in CLASSES_OF[c] + ("contig",):
        g, im = guarded(gpu, kind, arr)
        assert im.filter(VIGNETTE[0]) == 0
        in_place(gpu, g, im, chained(("smooth", 0), arr, VIGNETTE), ("vignette", c, kind), approx=True)


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("stage", ["rgb2hsv", "hsv2rgb"])
def test_hsv_stages_in_place(gpu, stage, c):
    for kind in CLASSES_OF[c]:
        for w, h in SMALL:
            arr = frame(w, h, c, 1)                                    # noise: any byte triple, hues past 180 among them
            g, im = guarded(gpu, kind, arr)
            assert getattr(im, stage)() == 0
            in_place(gpu, g, im, ref((stage, w, h, c), lambda: getattr(orc, stage)(arr)), (stage, c, kind, w, h))


@pytest.mark.parametrize("args", ["", "wide"])
def test_ascii_leaves_hsv_in_the_window_only(gpu, args):
    w, h = ASCII_SIZE
    arr = ref(("smooth", w, h, 3, 0), lambda: smooth_image(h, w, 3))
    for kind in CLASSES_OF[3]:
        g, im = guarded(gpu, kind, arr)
        text = im.ascii(args)
        assert text == ref(("ascii", args), lambda: orc.ascii_art(arr, args)), (args, kind)
        in_place(gpu, g, im, ref(("rgb2hsv", w, h, 3, "smooth"), lambda: orc.rgb2hsv(arr)), ("ascii", args, kind))


def test_blend_with_paper_in_place(gpu):
    for w, h in SMALL:
        arr = frame(w, h, 4, 2)
        for kind in ("a16", "a4"):
            g, im = guarded(gpu, kind, arr)
            assert im.blend_with_paper() == 0
            in_place(gpu, g, im, ref(("paper", w, h), lambda: orc.blend_with_paper(arr)), ("paper", kind, w, h))
        g, im = guarded(gpu, "a1", arr)
        refused(gpu, g, im, im.blend_with_paper(), ("paper", "a1", w, h))


def _overlay(size, sc, seed):
    ov = noise_image(size[1], size[0], sc, seed)
    if sc == 4:
        ov[:, :, 3] = np.linspace(0, 255, size[0]).astype(np.uint8)[None, :]
    return ov


# (overlay, gravity x, gravity y, offset x, offset y, opacity): inside the frame; clipped at the left and top, at the right
# and bottom, at the bottom alone; an overlay larger than the frame
PLACEMENTS = [(WM_OVERLAY, "r", "b", 16, 16, 60), (WM_OVERLAY, "l", "t", -20, -10, 50), (WM_OVERLAY, "r", "b", -10, -10, 80),
              (WM_OVERLAY, "c", "b", 0, 80, 1), (WM_HUGE, "l", "t", 0, 0, 70), (WM_HUGE, "c", "c", 3, -2, 40)]


@pytest.mark.parametrize("dc,sc", [(4, 4), (4, 3), (3, 4), (3, 3)])
def test_watermark_in_place(gpu, dc, sc):
    """k_blend_over chooses per pixel: BGRA under a BGRA overlay moves dwords where both addresses are on the 4-byte grid
    (a16, a4) and bytes where they are not -- the a1 window, which launch_blend_over does not refuse."""
    base = frame(WM_BASE[0], WM_BASE[1], dc, 3)
    kinds = CLASSES_OF[dc] + (("a1",) if (dc, sc) == (4, 4) else ())
    for size, gx, gy, ox, oy, op in PLACEMENTS:
        ov = _overlay(size, sc, 15)
        rc_o, want = ref(("wm", dc, sc, size, gx, gy, ox, oy, op), lambda: orc.watermark(base, ov, gx, gy, ox, oy, op))
        cfg = gpu.Config()
        assert cfg.prepare_watermark(ov, gx, gy, ox, oy, op) == 0
        try:
            for kind in kinds:
                where = (dc, sc, size, gx, gy, ox, oy, kind)
                g, im = guarded(gpu, kind, base)
                rc = im.watermark(cfg)
                assert rc == rc_o, (where, rc, rc_o)
                in_place(gpu, g, im, want if rc == 0 else base, where)
        finally:
            cfg.release()


def blur_case(gpu, c, size, sigma, kind, place, seed=4):
    """place: "window" (the blur worked in place), "fresh" (it wrote a frame of its own) or "refused"."""
    w, h = size
    arr = frame(w, h, c, seed)
    g, im = guarded(gpu, kind, arr)
    rc = im.filter("blur=%s" % sigma)
    where = ("blur", sigma, c, kind, w, h)
    if place == "refused":
        return refused(gpu, g, im, rc, where)
    assert rc == 0, (where, rc)
    want = ref(("gauss", w, h, c, seed, sigma), lambda: orc.gaussian(arr, float(np.float32(sigma))))
    if place == "window":
        in_place(gpu, g, im, want, where)
    else:
        assert not on_window(g, im), where
        fresh_frame(gpu, g, im, want, where)


@pytest.mark.parametrize("sigma", [2, 8])
def test_gray_blur_in_place(gpu, sigma):
    """launch_gaussian_fused takes colour frames only: a gray window is blurred where it lies."""
    for size in BLUR_SIZES:
        for kind in CLASSES_OF[1]:
            blur_case(gpu, 1, size, sigma, kind, "window")


@pytest.mark.parametrize("c", [1, 3, 4])
def test_thin_frames_blur_in_place(gpu, c):
    """One row or one column: no one-pass form, the blur drops that axis and works in place."""
    for size in THIN:
        for kind in CLASSES_OF[c]:
            blur_case(gpu, c, size, 2, kind, "window")
    if c == 4:
        for size in THIN:
            blur_case(gpu, 4, size, 2, "a1", "refused")


@pytest.mark.parametrize("c", [3, 4])
def test_widest_blurs(gpu, c):
    """sigma 31 trims to a radius of 60: the two-pass matrix-unit form still takes it (16 + 2 * cn * r <= 512 holds up to
    radius 62 for BGRA and 82 for BGR, blur_form says 3), so it writes a fresh frame and the window stays.  sigma 50 is past
    both limits and past the strips' 60: launch_gaussian_fused declines, launch_gaussian blurs the window in place.  BGRA
    off the 4-byte grid: the one-pass forms decline, launch_gaussian refuses."""
    for size in BLUR_SIZES:
        assert gpu.blur_form(size[0], size[1], c, 31.0) == (3, 2)
        assert gpu.blur_form(size[0], size[1], c, 50.0) == (0, 0)
        for kind in CLASSES_OF[c]:
            blur_case(gpu, c, size, 31, kind, "fresh")
            blur_case(gpu, c, size, 50, kind, "window")
        if c == 4:
            blur_case(gpu, 4, size, 31, "a1", "refused")
            blur_case(gpu, 4, size, 50, "a1", "refused")


# ================================================================= c. read a wrapped window, write a fresh frame
def filter_fresh(gpu, c, size, request_, kind, seed=5):
    w, h = size
    arr = frame(w, h, c, seed)
    g, im = guarded(gpu, kind, arr)
    rc = im.filter(request_)
    where = (request_, c, kind, w, h)
    assert rc == 0, (where, rc)
    fresh_frame(gpu, g, im, ref(("filter", w, h, c, seed, request_), lambda: orc.filter(arr, request_)[1]), where)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("request_", ["flip=10", "flip=01", "flip=11"])
def test_flip_reads_the_window_only(gpu, request_, c):
    for size in SMALL:
        for kind in CLASSES_OF[c]:
            filter_fresh(gpu, c, size, request_, kind)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("request_", ["rotate=90", "rotate=180", "rotate=270"])
def test_rotate_reads_the_window_only(gpu, request_, c):
    """BGR quarter turns move whole 32 x 32 tiles as dwords when source, destination, both pitches and the tile's first
    source column (in bytes) are on the 4-byte grid: 96 x 64 in a16 and a4 is all such tiles, in a1 none; 65 x 64 turned by
    270 has whole tiles that start 99 and 3 bytes into aligned rows and must take bytes."""
    for size in ROTATE_SIZES + ([ODD_COLUMN] if c == 3 else []):
        for kind in CLASSES_OF[c]:
            filter_fresh(gpu, c, size, request_, kind)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_crop_copies_out_of_the_window(gpu, c):
    """materialize: k_copy<4> for BGRA (dwords), k_copy_run for the BGR and gray windows, whose rows start anywhere."""
    w, h = SMALL[0]
    arr = frame(w, h, c, 6)
    rc_o, want = ref(("crop", c), lambda: orc.crop(arr, CROP))
    assert rc_o == 0 and want.shape == (17, 31, c)
    for kind in CLASSES_OF[c]:
        g, im = guarded(gpu, kind, arr)
        assert im.crop(CROP) == 0
        fresh_frame(gpu, g, im, want, ("crop", c, kind))


def test_gray2bgr_reads_the_window_only(gpu):
    for w, h in SMALL:
        arr = frame(w, h, 1, 7)
        for kind in CLASSES_OF[1]:
            g, im = guarded(gpu, kind, arr)
            assert im.gray2bgr() == 0
            fresh_frame(gpu, g, im, ref(("g2b", w, h), lambda: orc.gray2bgr(arr)), ("gray2bgr", kind, w, h))


# sigma -> impgpu_blur_form's (form, byte planes) at every size below, both channel counts.  Read from launch_gaussian_fused:
# radius 2 is k_blur_fused4 (form 1); from radius 3 on the matrix unit takes everything its chunk limits allow -- one pass
# (form 2: sigma 1 and 2 with two byte planes, sigma 4, whose taps sum to 258, with three) or, once a tile passes its LDS
# budget, two passes (form 3: sigma 12 and 20 with two planes, 10.5 with three).  k_blur_strip4 (radius 17 .. 60 where the
# matrix unit declines) is reached by no sigma at these channel counts, so 12 and 20 pin the two-pass form instead.
ONE_PASS = {"0.5": (1, 0), "1": (2, 2), "2": (2, 2), "4": (2, 3), "10.5": (3, 3), "12": (3, 2), "20": (3, 2)}


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("sigma", sorted(ONE_PASS, key=float))
def test_one_pass_blur_reads_the_window_only(gpu, sigma, c):
    """The parent is random: a border tap that read it instead of clamping to the window would miss the oracle.  200 x 9:
    every tap row clamps.  BGRA off the 4-byte grid is declined by every one-pass form and refused by launch_gaussian."""
    for size in ONE_PASS_SIZES:
        assert gpu.blur_form(size[0], size[1], c, float(sigma)) == ONE_PASS[sigma], (sigma, c, size)
        for kind in CLASSES_OF[c]:
            blur_case(gpu, c, size, sigma, kind, "fresh", seed=8)
        if c == 4:
            blur_case(gpu, 4, size, sigma, "a1", "refused", seed=8)


# ================================================================= d. the same through impgpu_batch_run_ops
# (job, config, works in place on a colour window)
JOBS = [(dict(filters=["gotham=1", "gamma=1.7"]), "plain", True),
        (dict(filters=["contrast=1.2"], need_flatten=1), "wm", True),
        (dict(filters=["flip=10"]), "plain", False),
        (dict(filters=["rotate=90"]), "plain", False),
        (dict(filters=["blur=2"]), "plain", False),
        (dict(filters=["blur=31"]), "plain", False),
        (dict(crop=CROP), "plain", False)]


def test_batch_run_ops_on_wrapped_windows(gpu):
    """One call over wrapped windows of every class, both colour channel counts and gray, four sizes.  Every request must
    come out as impgpu_run_ops leaves its twin (same bytes in a parent of its own) and as the oracle's chain; a request that
    still stands on its window worked in place and its window holds the answer, any other left its window as it was; no parent changes
    anywhere else."""
    from test_gpu_chain import oracle_chain

    ov = noise_image(9, 14, 4, 3050)
    wm = ("r", "b", 1, 1, 70)
    cfgs = {"plain": gpu.Config(allow_experiments=True), "wm": gpu.Config(allow_experiments=True)}
    assert cfgs["wm"].prepare_watermark(ov, *wm) == 0
    reqs = []
    for c in (1, 3, 4):
        for kind in CLASSES_OF[c]:
            for k, (job, cfg, stays) in enumerate(JOBS):
                w, h = BATCH_SIZES[(k + len(reqs)) % len(BATCH_SIZES)]
                reqs.append((frame(w, h, c, 30 + k), kind, job, cfg, stays and c != 1))
    parents, twins, ims, clones = [], [], [], []
    for i, (arr, kind, job, cfg, stays) in enumerate(reqs):
        for group, images in ((parents, ims), (twins, clones)):
            g, im = guarded(gpu, kind, arr, seed=i)
            group.append(g)
            images.append(im)
    try:
        res, launches = gpu.batch_run_ops(ims, [cfgs[r[3]] for r in reqs], [r[2] for r in reqs])
        loop = [gpu.run_ops(cl, cfgs[r[3]], **r[2]) for cl, r in zip(clones, reqs)]
        print("%d requests, %d launches" % (len(reqs), launches))
        for i, (arr, kind, job, cfg, stays) in enumerate(reqs):
            where = (i, arr.shape, kind, job)
            rc_o, step_o, want = oracle_chain(arr, overlay=ov if cfg == "wm" else None, wm=wm, flatten=job.get("need_flatten", 0),
                                              **{k: v for k, v in job.items() if k != "need_flatten"})
            assert res[i] == tuple(loop[i]) == (rc_o, step_o) == (0, 7), (where, res[i], loop[i])
            got, twin = ims[i].numpy(), clones[i].numpy()
            assert np.array_equal(got, twin), where
            assert got.shape == want.shape and np.array_equal(got, want), where
            for g, im in ((parents[i], ims[i]), (twins[i], clones[i])):
                kept = on_window(g, im)
                assert kept == stays, where
                rep = g.report(gpu, fresh=not kept)
                if kept:
                    assert np.array_equal(rep.windows[0].reshape(want.shape), want), where
                assert rep.intact, (where, describe(rep))
    finally:
        for im in ims + clones:
            im.release()
        for cfg in cfgs.values():
            cfg.release()
    del parents, twins


def layouts_used():
    """Every layout these tests build, for the host test of the helper: each kind at each size and channel count, alone and
    as a batch of three; the big batch; the refusal test's own."""
    for kind in KINDS:
        for w, h in ALL_SIZES:
            for c in (1, 3, 4):
                for count in (1, 3):
                    yield layout_for(kind, w, h, c, count)
    for c in (3, 4):
        yield layout_for("contig", BIG[0], BIG[1], c, BIG_COUNT)
    yield WindowLayout(VEC[0] * 4, VEC[1], 3, "a1", start="a16", stride_cls="a16")
    yield WindowLayout(VEC[0] * 4, VEC[1], 3, "a16", stride_cls="a1")
