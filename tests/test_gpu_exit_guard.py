"""The exits of a request under guard: the answer encoders (JPEG, GIF, PNG), the FreeImage and plain downloads and
CalcPerceivedBrightness read a frame and write an answer to host memory.  Here the frame is a wrapped window inside a parent of
random bytes (window_guard), in each alignment class an exit chooses its route by:

  JPEG  k_jpeg_enc_blocks: `aligned = !((src | step) & 3)` -- whole dwords for the blocks inside the frame, bytes with the last
        column repeated otherwise.  No class is refused: BGRA off the 4-byte grid takes the byte route, which reads B, G, R.
  GIF   gif_enc_key: `wide` (BGRA, src | step on the 4-byte grid) loads a dword per pixel, anything else three or four bytes.
        Gray is refused (IMP_ERROR_UNSUPPORTED) before anything is read.
  PNG   raw_at reads bytes only; the filters' "left of x = 0" and "above y = 0" are zeros, never the parent's bytes.
  FI    pack_fi_pixel: BGRA -> 32 bpp moves dwords and is refused off the 4-byte grid (IMP_ERROR_INVALID_ARGS, the bitmap keeps
        its fill); the other three pairs move bytes and take every class.
  plain impgpu_image_download and the album downloads copy step * h bytes and pick the rows on the host; k_gather_rows
        (impgpu_batch_download) moves dwords when source, destination and both pitches are on the 4-byte grid, bytes otherwise.
  brightness  br_load_px: a dword per BGRA pixel wherever it lies, bytes for BGR and gray.

Every answer equals the CPU definition's byte for byte (the oracle, the Python models, np.float32 equality) -- a misread still
gives a well-formed file of a plausible picture, so nothing less notices -- and afterwards every byte of the parent equals the
copy from before: an exit writes nothing into the caller's memory.  No window stands at the end of its allocation.

Shapes are (width, height)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
import png_enc_model as model
from test_gif_encode_host import OK, UNSUPPORTED, frame_of, model_file, palette
from test_gpu_operator_guard import INVALID_ARGS, frame, guarded, ref
from window_guard import GuardedParent, describe, layout_for

pytestmark = pytest.mark.gpu

CLASSES = ("a16", "a4", "a1")
FILL = 0xC7

# ---- the sizes (the host test of the helper checks that every layout built from them is in its class)
# JPEG: ragged blocks only; one whole MCU (aligned classes load only dwords); both routes in one frame, with a chroma block whose
# 16-pixel rows are ragged
JPEG_SMALL = [(7, 5), (16, 16), (37, 21)]
# (size, channels): 294 block slots -- k_jpeg_enc_huff_seg; 289 gray blocks -- the same; 2166 slots -- k_jpeg_enc_pack + _stuff
JPEG_LARGE = [((104, 104), 3), ((136, 136), 1), ((304, 304), 3)]
QUALITIES = (100, 75)                                # 100: no misread of one level is quantised away
GIF_SIZES = [(61, 33), (7, 5)]
GIF_SEGMENTS = (0, 256)                              # 61 x 33 = 2013 pixels: one segment, and eight
PNG_SIZES = [(61, 45), (1, 9), (9, 1)]
FI_SIZES = [(53, 37), (7, 5)]
PLAIN = (53, 37)
ALL_SIZES = sorted(set(JPEG_SMALL + [s for s, _ in JPEG_LARGE] + GIF_SIZES + PNG_SIZES + FI_SIZES + [PLAIN]))


def unchanged(gpu, g, where):
    """The exit only read: every byte of the parent, the window included, is as before."""
    rep = g.report(gpu, fresh=True)
    assert rep.intact, (where, describe(rep))


def windows(gpu, kind, frames, seed=0):
    """`frames` (same geometry) as the windows of ONE parent of `kind` -> (parent, [Image])."""
    h, w, c = frames[0].shape
    g = GuardedParent(layout_for(kind, w, h, c, len(frames)), frames, seed)
    return g, [g.wrap(gpu, w, h, c, i) for i in range(len(frames))]


def release(ims):
    for im in ims:
        if im is not None:
            im.release()


# ================================================================= JPEG encode
def jpeg_file(arr, q, key):
    rc, blob = ref(("exit-jpeg", key, q), lambda: orc.jpeg_encode(arr, q))
    assert rc == 0
    return blob


def jpeg_case(gpu, size, c, kind, seed):
    w, h = size
    arr = frame(w, h, c, seed)
    g, im = guarded(gpu, kind, arr)
    try:
        for q in QUALITIES:
            where = ("jpeg", w, h, c, kind, q)
            rc, got = im.encode_jpeg(q)
            assert rc == 0, (where, rc)
            want = jpeg_file(arr, q, (w, h, c, seed))
            assert got == want, (where, len(got), len(want))
            unchanged(gpu, g, where)
    finally:
        im.release()


@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("size", JPEG_SMALL, ids=lambda s: "%dx%d" % s)
def test_jpeg_encode_reads_the_window_only(gpu, size, c, kind):
    """a16 and a4 take the dword route wherever a block's 8 (chroma: 16) columns lie inside the frame and the byte route at
    the ragged right edge; a1 takes the byte route for everything, interior blocks and whole frames included.  Behind each row
    lie the parent's random bytes, not pool padding: a column taken from there instead of repeating the last one, or a dword
    shifted by a byte, misses the oracle's file."""
    jpeg_case(gpu, size, c, kind, 40)


@pytest.mark.parametrize("kind", ["a4", "a1"])
@pytest.mark.parametrize("size,c", JPEG_LARGE, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "c%d" % v)
def test_jpeg_encode_segmented_and_packed_kernels_read_the_window_only(gpu, size, c, kind):
    """The same k_jpeg_enc_blocks in front of the other two entropy stages: more than 256 block slots (segments of 256, a
    workgroup each) and more than 2048 (pack + stuff)."""
    jpeg_case(gpu, size, c, kind, 41)


def test_batch_encode_jpeg_over_windows(gpu):
    """One call over windows of every class and channel count -- three of one parent per class, the others in parents of their
    own, frames of all three entropy stages among them -- and a pool frame: each answer is its lone call's and the oracle's."""
    q = 100
    items = []                                                        # (key, frame, Image)
    parents = []
    for kind in CLASSES:
        w, h = JPEG_SMALL[2]
        frames = [frame(w, h, 3, 50 + i) for i in range(3)]
        g, ims = windows(gpu, kind, frames, seed=1)
        parents.append(g)
        items += [((w, h, 3, 50 + i), f, im) for i, (f, im) in enumerate(zip(frames, ims))]
    lone = [(kind, size, c, 40) for c in (1, 4) for kind, size in zip(CLASSES, JPEG_SMALL)]
    lone += [("a1", JPEG_SMALL[1], 3, 40), ("a4", JPEG_SMALL[0], 3, 40)]
    lone += [("a1", JPEG_LARGE[0][0], 3, 41), ("a4", JPEG_LARGE[1][0], 1, 41), ("a1", JPEG_LARGE[2][0], 3, 41)]
    for kind, (w, h), c, seed in lone:
        arr = frame(w, h, c, seed)
        g, im = guarded(gpu, kind, arr, seed=2)
        parents.append(g)
        items.append(((w, h, c, seed), arr, im))
    w, h = JPEG_SMALL[2]
    items.append(((w, h, 3, 53), frame(w, h, 3, 53), gpu.Image(frame(w, h, 3, 53))))            # a pool frame
    ims = [it[2] for it in items]
    try:
        got = gpu.batch_encode_jpeg(ims, q)
        alone = [im.encode_jpeg(q) for im in ims]
        for (key, arr, _), res, one in zip(items, got, alone):
            want = jpeg_file(arr, q, key)
            assert res[0] == one[0] == 0, (key, res[0], one[0])
            assert res[1] == one[1], key
            assert res[1] == want, (key, len(res[1]), len(want))
        for g in parents:
            unchanged(gpu, g, "batch jpeg")
    finally:
        release(ims)
    del parents


# ================================================================= GIF encode
def gif_frame(w, h, c):
    """At most 256 colours, every one of them present; BGRA: a fifth of the pixels transparent (alpha 0 over a colour of
    their own) and random alphas elsewhere."""
    def make():
        rng = np.random.default_rng(0x61F + w * 131 + h * 7 + c)
        colours = palette(rng, min(200, w * h // 2))
        f = frame_of(rng, w, h, colours, transparent=0.2 if c == 4 else 0.0, alpha=c == 4)
        assert f.shape == (h, w, c)
        return f
    return ref(("exit-gif-frame", w, h, c), make)


def gif_file(w, h, c, segment):
    return ref(("exit-gif", w, h, c, segment), lambda: model_file([gif_frame(w, h, c)], segment=segment))


@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("size", GIF_SIZES, ids=lambda s: "%dx%d" % s)
def test_gif_encode_reads_the_window_only(gpu, size, c, kind):
    """A single wrapped image is an album of one.  BGR: three byte loads in every class; BGRA in a16 and a4: `wide`, a dword
    per pixel; BGRA in a1: four byte loads.  segment 256 cuts the larger frame into eight LZW segments."""
    w, h = size
    arr = gif_frame(w, h, c)
    g, im = guarded(gpu, kind, arr)
    try:
        for segment in GIF_SEGMENTS:
            where = ("gif", w, h, c, kind, segment)
            want = gif_file(w, h, c, segment)
            assert want is not None
            rc, got, n, intact = gpu.encode_gif(im, segment=segment)
            assert rc == OK and intact and n == len(want), (where, rc, intact, n, len(want))
            assert got == want, where
            unchanged(gpu, g, where)
    finally:
        im.release()


@pytest.mark.parametrize("kind", CLASSES)
def test_gif_encode_refuses_a_gray_window(gpu, kind):
    """gif_enc_key reads three bytes per pixel whatever `channels` says, so a 1-channel image must never reach it:
    gif_enc_check_geometry refuses it (IMP_ERROR_UNSUPPORTED, length 0, nothing written) before anything is launched."""
    for w, h in GIF_SIZES:
        g, im = guarded(gpu, kind, frame(w, h, 1, 42))
        try:
            rc, got, n, intact = gpu.encode_gif(im, capacity=4096)
            assert rc == UNSUPPORTED and got is None and n == 0 and intact, (kind, w, h, rc, n, intact)
            rc, res, launches = gpu.batch_encode_gif([im], capacities=[4096])
            assert rc == OK and launches == 0 and res[0][0] == UNSUPPORTED and res[0][2] == 0 and res[0][3], (kind, w, h, rc, res[0][:1], launches)
            unchanged(gpu, g, ("gif gray", kind, w, h))
        finally:
            im.release()


def test_batch_encode_gif_over_windows(gpu):
    """Wide (a16, a4) and not-wide (a1) BGRA windows with BGR ones of every class in one call: each answer is its lone call's
    and the model's."""
    items = []
    parents = []
    for k, (c, kind) in enumerate([(4, "a16"), (3, "a1"), (4, "a1"), (3, "a16"), (4, "a4"), (3, "a4"), (4, "a1")]):
        w, h = GIF_SIZES[k % 2]
        g, im = guarded(gpu, kind, gif_frame(w, h, c), seed=k)
        parents.append(g)
        items.append(((w, h, c), im))
    ims = [im for _, im in items]
    try:
        lone = [gpu.encode_gif(im, segment=256) for im in ims]
        rc, results, launches = gpu.batch_encode_gif(ims, segment=256)
        assert rc == OK
        for ((w, h, c), _), res, one in zip(items, results, lone):
            want = gif_file(w, h, c, 256)
            assert res[0] == one[0] == OK and res[3] and one[3], (w, h, c, res[0], one[0])
            assert res[1] == one[1] and res[2] == one[2] == len(want), (w, h, c)
            assert res[1] == want, (w, h, c)
        for g in parents:
            unchanged(gpu, g, "batch gif")
    finally:
        release(ims)
    del parents


# ================================================================= PNG encode
def png_frame(content, w, h, c):
    return ref(("exit-png-frame", content, w, h, c), lambda: model.make_frame(content, h, w, c, 3 + c))


def png_file(content, w, h, c):
    return ref(("exit-png", content, w, h, c), lambda: model.encode(png_frame(content, w, h, c)))


@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("content", ["noise", "smooth"])
def test_png_encode_reads_the_window_only(gpu, content, c, kind):
    """Sub, Average and Paeth read the pixel to the left, Up, Average and Paeth the row above: at x = 0 and y = 0 those are
    zeros, and in a window the byte that lies there is the parent's, random.  On the smooth frame the filter chosen varies
    from row to row, so a wrong sum at the left edge changes the choice; one column and one row are the shapes at which
    libpng drops filters.  The kernel reads bytes: every class is taken, BGRA off the 4-byte grid too."""
    for w, h in PNG_SIZES:
        where = ("png", content, w, h, c, kind)
        arr = png_frame(content, w, h, c)
        g, im = guarded(gpu, kind, arr)
        try:
            rc, got = im.encode_png(9)
            assert rc == 0, (where, rc)
            assert got == png_file(content, w, h, c), where
            unchanged(gpu, g, where)
        finally:
            im.release()


def test_batch_encode_png_over_windows(gpu):
    """One call over windows of every class and channel count (three of one parent among them) and a pool frame."""
    items = []
    parents = []
    w, h = PNG_SIZES[0]
    frames = [png_frame("smooth", w, h, 3), png_frame("noise", w, h, 3), png_frame("smooth", w, h, 3)]
    g, ims = windows(gpu, "a1", frames, seed=3)
    parents.append(g)
    items += [(("smooth", w, h, 3), ims[0]), (("noise", w, h, 3), ims[1]), (("smooth", w, h, 3), ims[2])]
    k = 0
    for c in (1, 3, 4):
        for kind in CLASSES:
            content = ("smooth", "noise")[k % 2]
            w, h = PNG_SIZES[k % 3]
            g, im = guarded(gpu, kind, png_frame(content, w, h, c), seed=4)
            parents.append(g)
            items.append(((content, w, h, c), im))
            k += 1
    w, h = PNG_SIZES[0]
    items.append((("smooth", w, h, 4), gpu.Image(png_frame("smooth", w, h, 4))))                # a pool frame
    ims = [im for _, im in items]
    try:
        got = gpu.batch_encode_png(ims, 9)
        alone = [im.encode_png(9) for im in ims]
        for (key, _), res, one in zip(items, got, alone):
            assert res[0] == one[0] == 0, (key, res[0], one[0])
            assert res[1] == one[1], key
            assert res[1] == png_file(*key), key
        for g in parents:
            unchanged(gpu, g, "batch png")
    finally:
        release(ims)
    del parents


# ================================================================= FreeImage download
def fi_bitmap(w, h, c, bpp):
    return ref(("exit-fi", w, h, c, bpp), lambda: orc.ipl_to_fi(frame(w, h, c, 43), bpp))


def fi_pitches(w, bpp):
    own = (w * bpp // 8 + 3) & ~3
    return own, own + 8


def fi_refused(c, bpp, kind):
    return c == 4 and bpp == 32 and kind == "a1"


def fi_check(got, w, h, c, bpp, pitch, accepted, where):
    rowbytes = w * bpp // 8
    assert got.shape == (h, pitch), where
    if accepted:
        assert np.array_equal(got[:, :rowbytes], fi_bitmap(w, h, c, bpp)[:, :rowbytes]), where
        assert (got[:, rowbytes:] == FILL).all(), where                  # the bytes between the rows are the caller's
    else:
        assert (got == FILL).all(), where


@pytest.mark.parametrize("kind", CLASSES)
@pytest.mark.parametrize("bpp", [24, 32])
@pytest.mark.parametrize("c", [3, 4])
def test_download_fi_reads_the_window_only(gpu, c, bpp, kind):
    """BGRA -> 32 bpp moves a dword per pixel: refused where the window is off the 4-byte grid (IMP_ERROR_INVALID_ARGS, the
    bitmap keeps its fill).  BGRA -> 24, BGR -> 24 and BGR -> 32 move bytes and take every class."""
    for w, h in FI_SIZES:
        g, im = guarded(gpu, kind, frame(w, h, c, 43))
        try:
            for pitch in fi_pitches(w, bpp):
                where = ("fi", w, h, c, bpp, kind, pitch)
                rc, outs = im.frames_fi(bpp, pitch, fill=FILL)
                accepted = not fi_refused(c, bpp, kind)
                assert rc == (0 if accepted else INVALID_ARGS), (where, rc)
                assert len(outs) == 1, where
                fi_check(outs[0], w, h, c, bpp, pitch, accepted, where)
                unchanged(gpu, g, where)
        finally:
            im.release()


def test_batch_download_fi_over_windows(gpu):
    """Every (channels, bpp, class, size, pitch) of the lone test in one call: only the BGRA -> 32 bpp windows off the 4-byte
    grid are refused, each alone."""
    specs = [(c, bpp, kind, size, which) for c in (3, 4) for bpp in (24, 32) for kind in CLASSES for size in FI_SIZES for which in (0, 1)]
    parents, ims, pitches = [], [], []
    for k, (c, bpp, kind, (w, h), which) in enumerate(specs):
        g, im = guarded(gpu, kind, frame(w, h, c, 43), seed=k)
        parents.append(g)
        ims.append(im)
        pitches.append(fi_pitches(w, bpp)[which])
    try:
        outs, codes, launches = gpu.batch_download_fi(ims, [s[1] for s in specs], pitches, fill=FILL)
        assert launches == 4, launches                                   # one per (channels, bpp) pair
        refused = 0
        for (c, bpp, kind, (w, h), which), out, code, pitch in zip(specs, outs, codes, pitches):
            where = ("batch fi", w, h, c, bpp, kind, pitch)
            accepted = not fi_refused(c, bpp, kind)
            refused += not accepted
            assert code == (0 if accepted else INVALID_ARGS), (where, code)
            assert len(out) == 1, where
            fi_check(out[0], w, h, c, bpp, pitch, accepted, where)
        assert refused == 4
        for g in parents:
            unchanged(gpu, g, "batch fi")
    finally:
        release(ims)
    del parents


# ================================================================= plain download and brightness
def plain_windows(gpu):
    """-> (parents, Images, frames): a 53 x 37 window per class and channel count."""
    w, h = PLAIN
    parents, ims, frames = [], [], []
    for c in (1, 3, 4):
        for kind in CLASSES:
            arr = frame(w, h, c, 44)
            g, im = guarded(gpu, kind, arr, seed=c)
            parents.append(g); ims.append(im); frames.append(arr)
    return parents, ims, frames


def test_download_reads_the_window_only(gpu):
    """impgpu_image_download, impgpu_album_download and impgpu_batch_album_download (the rows picked out of one copy of
    step * h bytes) and impgpu_batch_download into ordinary memory (k_gather_rows: dwords for a16 and a4, bytes for a1; 53
    gray bytes and 159 BGR bytes a row leave a tail of bytes behind the dwords), with the caller's own pitch."""
    parents, ims, frames = plain_windows(gpu)
    try:
        for g, im, arr in zip(parents, ims, frames):
            got = im.numpy()
            assert got.shape == arr.shape and np.array_equal(got, arr), arr.shape
            one = im.frames()                                            # impgpu_album_download: an album of one
            assert len(one) == 1 and np.array_equal(one[0], arr), arr.shape
        many, codes = gpu.batch_album_download(ims)
        assert codes == [0] * len(ims), codes
        for arr, mine in zip(frames, many):
            assert len(mine) == 1 and np.array_equal(mine[0], arr), arr.shape
        n = len(ims)
        rowbytes = [a.shape[1] * a.shape[2] for a in frames]
        outs = [np.full((a.shape[0], rb + 5), FILL, np.uint8) for a, rb in zip(frames, rowbytes)]
        handles = (C.c_void_p * n)(*[im.h.value for im in ims])
        datas = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        steps = (C.c_int * n)(*[o.shape[1] for o in outs])
        assert gpu.lib.impgpu_batch_download(handles, n, datas, steps) == 0
        for arr, rb, o in zip(frames, rowbytes, outs):
            assert np.array_equal(o[:, :rb].reshape(arr.shape), arr), arr.shape
            assert (o[:, rb:] == FILL).all(), arr.shape
        for g in parents:
            unchanged(gpu, g, "download")
    finally:
        release(ims)
    del parents


def test_batch_download_into_pinned_memory_reads_the_window_only(gpu):
    """Destinations the device can write get their rows straight from k_gather_rows, whose `words` asks source AND
    destination: every window goes once to a start and pitch on the 4-byte grid (dwords for a16 and a4, bytes for a1) and once
    to an odd start with an odd pitch (bytes for all).  Nothing but the rows is written there, nothing at all in the parents."""
    parents, ims, frames = plain_windows(gpu)
    plan = []                                                         # (window, offset, pitch)
    at = 0
    for k, arr in enumerate(frames):
        rb = arr.shape[1] * arr.shape[2]
        for pitch, shift in (((rb + 8 + 3) & ~3, 0), ((rb + 5) | 1, 1)):
            plan.append((k, at + shift, pitch))
            at = (at + shift + arr.shape[0] * pitch + 64 + 3) & ~3
    total = at + 64
    base = gpu.lib.impgpu_host_alloc(total)
    assert base and base % 4 == 0
    try:
        buf = np.ctypeslib.as_array((C.c_ubyte * total).from_address(base))
        buf[:] = FILL
        n = len(plan)
        handles = (C.c_void_p * n)(*[ims[k].h.value for k, _, _ in plan])
        datas = (C.c_void_p * n)(*[base + off for _, off, _ in plan])
        steps = (C.c_int * n)(*[pitch for _, _, pitch in plan])
        assert gpu.lib.impgpu_batch_download(handles, n, datas, steps) == 0
        touched = np.zeros(total, dtype=bool)
        for k, off, pitch in plan:
            arr = frames[k]
            h, rb = arr.shape[0], arr.shape[1] * arr.shape[2]
            view = buf[off: off + h * pitch].reshape(h, pitch)
            assert np.array_equal(view[:, :rb].reshape(arr.shape), arr), (arr.shape, off, pitch)
            for y in range(h):
                touched[off + y * pitch: off + y * pitch + rb] = True
        assert np.all(buf[~touched] == FILL)
        for g in parents:
            unchanged(gpu, g, "pinned download")
        del buf
    finally:
        gpu.lib.impgpu_host_free(C.c_void_p(base))
        release(ims)
    del parents


def test_brightness_reads_the_window_only(gpu):
    """CalcPerceivedBrightness alone and impgpu_batch_calc_perceived_brightness over the same windows: the oracle's float,
    bit for bit.  No class is refused: a BGRA pixel is one dword load wherever it lies."""
    parents, ims, frames = plain_windows(gpu)
    try:
        want = [np.float32(ref(("exit-brightness", a.shape), lambda: orc.brightness(a))) for a in frames]
        lone = [im.calc_perceived_brightness() for im in ims]
        vals, codes, launches = gpu.batch_calc_perceived_brightness(ims)
        assert codes == [0] * len(ims), codes
        for a, w_, one, v in zip(frames, want, lone, vals):
            assert np.float32(one) == w_, (a.shape, one, w_)
            assert np.float32(v) == w_, (a.shape, v, w_)
        for g in parents:
            unchanged(gpu, g, "brightness")
    finally:
        release(ims)
    del parents


def layouts_used():
    """Every layout these tests build, for the host test of the helper: each class at each size and channel count, alone and
    as the three windows of one parent."""
    for kind in CLASSES:
        for w, h in ALL_SIZES:
            for c in (1, 3, 4):
                for count in (1, 3):
                    yield layout_for(kind, w, h, c, count)
