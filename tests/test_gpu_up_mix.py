"""CUBIC enlargements of different geometry share a launch (launch_resize_mixed's MIX_UP class, k_resize_up_cubic_mix).

The mix kernel carries the bodies of the lone enlargement kernels behind a descriptor table and the frames' tables travel
with the launch, so every output must equal, byte for byte, what one impgpu_batch_cv_resize launch per frame leaves and what
the oracle's INTER_CUBIC computes -- and the number of kernels enqueued must follow the kinds of frames in a call, not
their number."""
import math

import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_int_mix import CANARY, Frame, _check_frames
from test_gpu_mixed_classes import Placed

pytestmark = pytest.mark.gpu

A, CUBIC = orc.INTER_AREA, orc.INTER_CUBIC
UP_ROWS, UP_CAP_PX, UP_CAP3_BYTES = 128, 1536, 6144        # imp_resize.hip


def takes(cn, sw, sh, dw, dh):
    """up_cubic_takes of imp_resize.hip for a frame Resize() sends to CUBIC (the 2^32 bound is out of reach here)."""
    scale_x, scale_y = 1. / (dw / sw), 1. / (dh / sh)
    return cn in (3, 4) and (dw > sw or dh > sh) and scale_y <= 1.0 and scale_x <= 2.0 and sw >= 4


def rows_per_wave(cn, sw, sh, dw, dh, frames):
    """up_rows_per_wave of imp_resize.hip."""
    scale_x, scale_y = 1. / (dw / sw), 1. / (dh / sh)
    nbx = (dw + 255) // 256
    wmax = math.floor(63 * scale_x) + 6
    pitch, cap = ((((wmax * 3 + 3) & ~3) + 4), UP_CAP3_BYTES) if cn == 3 else (wmax, UP_CAP_PX)
    rpw = UP_ROWS
    while rpw > 4 and (math.floor((rpw - 1) * scale_y) + 6) * pitch > cap:
        rpw -= 4
    while rpw > 16 and nbx * 4 * ((dh + rpw - 1) // rpw) * frames < 8192:
        rpw -= 64 if rpw > 64 else 16
    return rpw


class UpFrame(Frame):
    """test_gpu_int_mix.Frame with everything chosen, not drawn: the source window's first column, the destination's canary
    columns (`dpad`) and `below` canary rows under the destination."""

    def __init__(self, torch, rng, cn, shape, interp=CUBIC, ox=4, dpad=None, below=0):
        sw, sh, dw, dh = shape
        self.cn, self.sw, self.sh, self.dw, self.dh, self.interp, self.below = cn, sw, sh, dw, dh, interp, below
        dpad = (-dw) % 4 if dpad is None else dpad           # default: rows on the 16-byte (BGR: 4-byte) grid
        px = (-(sw + ox)) % 4
        self.host = rng.integers(0, 256, size=(sh + 3, sw + ox + px, cn), dtype=np.uint8)
        self.window = self.host[2:2 + sh, ox:ox + sw]
        self.src = torch.from_numpy(self.host).cuda()
        self.sstep = self.host.shape[1] * cn
        self.sptr = self.src.data_ptr() + 2 * self.sstep + ox * cn
        self.dsts = [torch.full((dh + below, dw + dpad, cn), CANARY, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.dstep = (dw + dpad) * cn

    def out(self, which):
        return self.dsts[which].cpu().numpy()[:self.dh]

    def under(self, which):
        return self.dsts[which].cpu().numpy()[self.dh:]


# (sw, sh, dw, dh) and what each is there for
SMALLEST = (4, 4, 5, 7)                # the smallest source the rule takes; one partial strip; dword path only
FOURFOLD = (40, 10, 128, 40)           # two full strips, whole groups of four rows: the patch stores; y factor exactly 4
ODD = (33, 9, 131, 23)                 # odd width: the scalar tail in the last strip (3 live lanes); dh % 4 != 0
TWO_BLOCKS = (70, 9, 300, 20)          # nbx = 2: the second workgroup has one partial wave and three that return
X_SHRINKS = (520, 12, 261, 13)         # x shrinks by 1.99 while y grows: the LDS bound cuts the chunk
CHUNKS = (30, 50, 64, 150)             # several row chunks: the footprint is re-primed at each chunk's first row
WHOLE = [(20, 20, 40, 40), (20, 20, 60, 60), (20, 20, 80, 80)]
ONE_AXIS = [(100, 80, 101, 80), (100, 80, 100, 81)]
ANY_SOURCE = (37, 11, 90, 30)          # a source window at an odd column (BGR: an odd byte and an odd pitch)
OUTSIDE = [(3, 5, 9, 11), (64, 48, 65, 30), (200, 10, 90, 11)]       # sw < 4; y shrinks; scale_x > 2
GENERAL = [(97, 61, 40, 25), (120, 50, 33, 21)]
WHOLE_SHRINKS = [(64, 48, 32, 24), (96, 60, 32, 20)]


def test_the_shapes_are_what_they_claim():
    accepted = [SMALLEST, FOURFOLD, ODD, TWO_BLOCKS, X_SHRINKS, CHUNKS, ANY_SOURCE] + WHOLE + ONE_AXIS
    for cn in (3, 4):
        assert all(takes(cn, *s) for s in accepted)
        assert not any(takes(cn, *s) for s in OUTSIDE)
        assert all(dw > sw or dh > sh for sw, sh, dw, dh in OUTSIDE)          # CUBIC all the same (bridge.c:188-192)
        assert all(dw <= 300 and dh <= 150 for _, _, dw, dh in accepted)
    assert not takes(1, *FOURFOLD)                                            # gray enlargements go alone
    sw, sh, dw, dh = SMALLEST
    assert sw == 4 and not takes(4, 3, sh, dw, dh) and dw < 64
    sw, sh, dw, dh = FOURFOLD
    assert dw == 2 * 64 and dh == 4 * sh and dh % 4 == 0
    sw, sh, dw, dh = ODD
    assert dw % 2 == 1 and dw % 64 == 3 and dh % 4 != 0
    assert all((dw * cn) & ~7 < dw * cn and (dw - 3) * cn <= (dw * cn) & ~7 for cn in (3, 4))   # a scalar tail, inside the last strip
    sw, sh, dw, dh = TWO_BLOCKS
    assert (dw + 255) // 256 == 2 and 0 < dw - 256 < 64
    # the LDS bound alone (a call of any size: the chip-fill rule starts above 16 rows) cuts the chunk to 4 rows for BGRA;
    # a BGR patch holds bytes, a third more pixels, and its bound is 8 rows: both make several chunks of the 13 rows
    sw, sh, dw, dh = X_SHRINKS
    assert 1.9 < sw / dw <= 2.0 and dh > sh
    assert [rows_per_wave(4, sw, sh, dw, dh, n) for n in (1, 10 ** 6)] == [4, 4]
    assert [rows_per_wave(3, sw, sh, dw, dh, n) for n in (1, 10 ** 6)] == [8, 8]
    sw, sh, dw, dh = CHUNKS
    assert all(rows_per_wave(cn, sw, sh, dw, dh, n) * 3 <= dh for cn in (3, 4) for n in (1, 2, 40))
    assert [dw // sw for sw, _, dw, _ in WHOLE] == [2, 3, 4] and all(dw == k * sw and dh == k * sh for k, (sw, sh, dw, dh) in zip((2, 3, 4), WHOLE))
    assert ONE_AXIS[0][1] == ONE_AXIS[0][3] and ONE_AXIS[0][2] > ONE_AXIS[0][0]
    assert ONE_AXIS[1][0] == ONE_AXIS[1][2] and ONE_AXIS[1][3] > ONE_AXIS[1][1]
    assert all(sw % dw == 0 and sh % dh == 0 for sw, sh, dw, dh in WHOLE_SHRINKS)
    assert all((sw % dw or sh % dh) and dw < sw and dh < sh for sw, sh, dw, dh in GENERAL)


def _odd_bgr(torch, rng):
    """A BGR source window that starts at an odd byte of rows with an odd pitch (Placed draws the window's first row: with
    an odd pitch every other draw gives an odd start)."""
    while True:
        f = Placed(torch, rng, 3, ANY_SOURCE, CUBIC, aligned=False)
        if f.sptr % 2 == 1:
            return f


def _accepted(torch, rng, cn):
    """Every accepted shape once, interleaved so that no two neighbours share a geometry."""
    frames = [UpFrame(torch, rng, cn, SMALLEST, dpad=3),
              UpFrame(torch, rng, cn, FOURFOLD, below=2),                     # on the grid: the four-row patch stores
              UpFrame(torch, rng, cn, WHOLE[0]),
              UpFrame(torch, rng, cn, ODD, dpad=2),
              UpFrame(torch, rng, cn, FOURFOLD, dpad=1, below=1),             # off the grid: the fast path must decline
              UpFrame(torch, rng, cn, TWO_BLOCKS),
              UpFrame(torch, rng, cn, WHOLE[1]),
              UpFrame(torch, rng, cn, X_SHRINKS, dpad=3, below=1),
              UpFrame(torch, rng, cn, ONE_AXIS[0]),
              UpFrame(torch, rng, cn, CHUNKS, below=1),
              UpFrame(torch, rng, cn, WHOLE[2]),
              UpFrame(torch, rng, cn, ONE_AXIS[1], dpad=1),
              _odd_bgr(torch, rng) if cn == 3 else UpFrame(torch, rng, cn, ANY_SOURCE, ox=1)]
    on_grid, off_grid = frames[1], frames[4]
    assert on_grid.dsts[0].data_ptr() % 16 == 0 and on_grid.dstep % (16 if cn == 4 else 4) == 0
    assert off_grid.dstep % (16 if cn == 4 else 4) != 0
    if cn == 4:
        assert frames[-1].sptr % 8 == 4                                       # an odd column
    else:
        assert frames[-1].sptr % 2 == 1 and frames[-1].sstep % 2 == 1         # an odd byte, an odd pitch
    return frames


def _check(gpu, frames, cn, where):
    _check_frames(gpu, frames, cn, where)
    for i, f in enumerate(frames):
        if getattr(f, "below", 0):
            assert (f.under(0) == CANARY).all() and (f.under(1) == CANARY).all(), (where, i)


@pytest.mark.parametrize("cn", [3, 4])
def test_every_accepted_shape_in_one_launch(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB100 + cn))
    frames = _accepted(torch, rng, cn)
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    print("cn %d: %d enlargements, %d launches" % (cn, len(frames), launches))
    assert rc == 0
    _check(gpu, frames, cn, "accepted")
    assert launches == 1, launches                                            # before the class existed: one each


@pytest.mark.parametrize("cn", [3, 4])
def test_enlargements_among_shrinks_and_frames_outside_the_rule(gpu, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB200 + cn))
    frames = _accepted(torch, rng, cn)
    others = [UpFrame(torch, rng, cn, s, A) for s in GENERAL + WHOLE_SHRINKS] + [UpFrame(torch, rng, cn, s, below=1) for s in OUTSIDE]
    for k, f in enumerate(others):
        frames.insert(2 * k + 1, f)
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    print("cn %d: %d frames, %d launches" % (cn, len(frames), launches))
    assert rc == 0
    _check(gpu, frames, cn, "among others")
    assert launches == 1 + 2 + 3, launches        # the enlargements; general and whole-factor shrinks; three frames alone


def test_two_share_one_alone_gray_each(gpu):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB300))
    for cn in (3, 4):
        two = [UpFrame(torch, rng, cn, ODD), UpFrame(torch, rng, cn, CHUNKS)]
        torch.cuda.synchronize()
        rc, launches = gpu.batch_resize_mixed([f.item(0) for f in two], cn, count_launches=True)
        assert (rc, launches) == (0, 1)
        _check(gpu, two, cn, "two")
        one = [UpFrame(torch, rng, cn, FOURFOLD, below=1)]                    # a class of one: the lone launch (PS = 4)
        torch.cuda.synchronize()
        rc, launches = gpu.batch_resize_mixed([f.item(0) for f in one], cn, count_launches=True)
        assert (rc, launches) == (0, 1)
        _check(gpu, one, cn, "one")
    gray = [UpFrame(torch, rng, 1, s) for s in (ODD, CHUNKS, FOURFOLD, WHOLE[0])]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in gray], 1, count_launches=True)
    assert (rc, launches) == (0, len(gray))                                   # as before: gray enlargements are not gathered
    _check(gpu, gray, 1, "gray")


@pytest.mark.parametrize("cn", [3, 4])
def test_same_size_avatars_share_one_launch(gpu, cn):
    """Forty frames of one geometry, and two of other geometries, share a launch; the lone launches _check_frames makes
    afterwards -- of that geometry and of the two others the mix used -- give the same bytes."""
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB400 + cn))
    frames = [UpFrame(torch, rng, cn, (20, 20, 64, 64)) for _ in range(40)]
    frames += [UpFrame(torch, rng, cn, (21, 19, 50, 47)), UpFrame(torch, rng, cn, (23, 17, 61, 40))]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    assert (rc, launches) == (0, 1)
    _check(gpu, frames, cn, "avatars")


def test_300_geometries_in_one_launch_then_the_lone_paths(gpu):
    """300 distinct enlargements in one launch, on the env stream and on a caller's; their lone launches (which run the
    256-entry table cache over) and 300 distinct AREA shrinks afterwards give the right bytes.  What the cache holds is not
    observed here: launch_up_mix never calls get_tables."""
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB500))
    geoms = []
    for i in range(300):
        sw, sh = 4 + i % 21, 4 + (i // 21) % 21
        geoms.append((sw, sh, min(40, sw + 1 + i % 16), min(40, sh + (i * 7) % 17)))
    assert len(set(geoms)) == 300 and all(takes(4, *g) for g in geoms)
    frames = [Frame(torch, rng, 4, *g, CUBIC) for g in geoms]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], 4, count_launches=True)
    assert (rc, launches) == (0, 1)
    _check_frames(gpu, frames, 4, "300")                   # (its 300 lone launches run the cache over: 256 entries)
    # the same call on a caller's stream
    for f in frames:
        f.dsts[0].fill_(CANARY)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], 4, stream=stream.cuda_stream, count_launches=True)
    assert (rc, launches) == (0, 1)
    stream.synchronize()
    for i, f in enumerate(frames):
        assert np.array_equal(f.out(0), f.out(1)), ("caller's stream", i)
    # the table cache still serves the lone paths: 300 distinct AREA shrinks on the env stream
    shrinks = [Frame(torch, rng, 4, 60 + i % 41, 40 + (i // 41) % 23, 11 + i % 13, 9 + i % 11, A) for i in range(300)]
    assert len({(f.sw, f.sh, f.dw, f.dh) for f in shrinks}) == 300
    torch.cuda.synchronize()
    assert gpu.batch_resize_mixed([f.item(0) for f in shrinks], 4) == 0
    _check_frames(gpu, shrinks, 4, "300 shrinks")


@pytest.mark.parametrize("bad", ["null_dst", "zero_width", "short_pitch"])
def test_a_malformed_item_launches_nothing(gpu, bad):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB600))
    frames = [UpFrame(torch, rng, 4, s) for s in (ODD, CHUNKS, FOURFOLD, WHOLE[1], TWO_BLOCKS)]
    torch.cuda.synchronize()
    items = [list(f.item(0)) for f in frames]
    if bad == "null_dst":
        items[3][4] = 0
    elif bad == "zero_width":
        items[3][1] = 0
    else:
        items[3][7] = items[3][5] * 4 - 4                                     # destination pitch shorter than a row
    rc, launches = gpu.batch_resize_mixed([tuple(it) for it in items], 4, count_launches=True)
    gpu.sync()
    assert rc == gpu.IMP_ERROR_INVALID_ARGS and launches == 0, (rc, launches)
    for f in frames:
        assert (f.dsts[0].cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("cn", [3, 4])
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(gpu, seed, cn):
    import torch

    rng = np.random.Generator(np.random.PCG64(0x1A4DB700 + 16 * seed + cn))
    n = int(rng.integers(2, 49))
    frames, outside = [], 0
    while len(frames) < n:
        dw, dh = int(rng.integers(1, 301)), int(rng.integers(1, 61))
        kind = int(rng.integers(0, 6))                     # mostly both axes grow; sometimes one shrinks
        fx = rng.uniform(0.15, 1.0) if kind != 4 else rng.uniform(1.0, 2.6)
        fy = rng.uniform(0.15, 1.0) if kind != 5 else rng.uniform(1.0, 2.6)
        sw, sh = max(1, int(dw * fx)), max(1, int(dh * fy))
        if not (dw > sw or dh > sh):
            continue
        frames.append(Frame(torch, rng, cn, sw, sh, dw, dh, CUBIC))
        outside += not takes(cn, sw, sh, dw, dh)
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], cn, count_launches=True)
    print("seed %d cn %d: %d frames (%d outside the rule), %d launches" % (seed, cn, n, outside, launches))
    assert rc == 0
    assert 1 <= launches <= 1 + outside, (n, outside, launches)
    _check_frames(gpu, frames, cn, "fuzz seed %d" % seed)
