"""impgpu_batch_download_fi / impgpu_batch_album_download: the FreeImage and the frame exits of many handles -- albums and single
images, 3 and 4 channels, 24 and 32 bits mixed -- behind one wait, the repack of every frame in one launch per (source
channels, bpp) pair (k_pack_fi_mix).  Expected bytes are the lone calls' and the oracle's IplToFI32 / IplToFI24."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image, smooth_image
from test_gif import random_album

pytestmark = pytest.mark.gpu

GUARD = 0xC7


def _album(gpu, c, frames, w, h, seed):
    """(Image, its frames as arrays): a GIF compose for BGRA albums, an uploaded album or single image otherwise."""
    if c == 4 and frames > 1:
        pages = random_album(seed, frames, w, h)
        rc, im = gpu.gif_compose(pages, bool(seed & 1), album=True)
        rc_o, arrs = orc.gif_compose(pages, bool(seed & 1))
        assert rc == 0 and rc_o == 0
        return im, arrs
    arrs = [smooth_image(h, w, 4, seed + f) if c == 4 else noise_image(h, w, c, seed + f) for f in range(frames)]
    return (gpu.Image.album(arrs) if frames > 1 else gpu.Image(arrs[0])), arrs


def _check(gpu, ims, arrs, bpps, pitches, outs, codes):
    for i, (im, frames, bpp) in enumerate(zip(ims, arrs, bpps)):
        assert codes[i] == 0 and len(outs[i]) == len(frames), i
        rc, lone = im.frames_fi(bpp, pitches[i], fill=GUARD)
        assert rc == 0
        rowbytes = frames[0].shape[1] * bpp // 8
        for f, (got, alone, a) in enumerate(zip(outs[i], lone, frames)):
            want = orc.ipl_to_fi(a, bpp)
            assert got.shape == alone.shape, (i, f)
            assert np.array_equal(got[:, :rowbytes], alone[:, :rowbytes]), (i, f)
            assert np.array_equal(got[:, :rowbytes], want[:, :rowbytes]), (i, f)
            assert (got[:, rowbytes:] == GUARD).all(), (i, f)                   # the bytes between the rows are the caller's


# (channels, frames, width, height, bpp, extra pitch): odd widths, rows whose step is not width * channels, several workgroups
# per frame (64 x 48 = 12 x 256 pixels) and frames of less than one
MIXED = [(4, 3, 37, 23, 32, 0), (4, 2, 20, 9, 24, 0), (3, 4, 33, 21, 32, 12), (3, 2, 50, 30, 24, 5), (4, 1, 45, 31, 24, 0),
         (3, 1, 41, 27, 32, 0), (4, 5, 64, 48, 32, 8), (3, 1, 7, 3, 24, 3), (4, 1, 5, 3, 32, 0), (3, 3, 64, 48, 24, 0)]


def test_mixed_handles_match_the_lone_calls_and_the_oracle(gpu):
    ims, arrs, bpps, pitches = [], [], [], []
    for k, (c, frames, w, h, bpp, extra) in enumerate(MIXED):
        im, a = _album(gpu, c, frames, w, h, 6000 + 10 * k)
        ims.append(im); arrs.append(a); bpps.append(bpp)
        pitches.append(((w * bpp // 8 + 3) & ~3) + extra)
    outs, codes, launches = gpu.batch_download_fi(ims, bpps, pitches, fill=GUARD)
    print("%d handles, %d frames, %d launches" % (len(ims), sum(len(o) for o in outs), launches))
    _check(gpu, ims, arrs, bpps, pitches, outs, codes)
    assert 1 <= launches <= 4, launches                                          # all four (channels, bpp) pairs are present
    assert launches == len({(c, bpp) for c, _, _, _, bpp, _ in MIXED})
    for im in ims:
        im.release()


def test_a_uniform_call_is_one_launch(gpu):
    ims, arrs = [], []
    for k in range(8):
        im, a = _album(gpu, 4, 2 + k % 4, 21 + 6 * k, 11 + 5 * k, 6200 + 10 * k)
        ims.append(im); arrs.append(a)
    outs, codes, launches = gpu.batch_download_fi(ims, [32] * 8, fill=GUARD)
    _check(gpu, ims, arrs, [32] * 8, [None] * 8, outs, codes)
    assert launches == 1, launches
    for im in ims:
        im.release()


def test_refused_entries_are_refused_alone(gpu):
    """A NULL handle (it owns no bitmaps), a gray image and a bpp of 16 in the middle: IMP_ERROR_INVALID_ARGS for them, their
    bitmaps untouched, everybody else served."""
    specs = [(4, 2, 37, 23, 32), None, (1, 1, 33, 21, 32), (3, 3, 33, 21, 24), (4, 1, 20, 9, 16), (3, 1, 41, 27, 32)]
    ims, arrs, bpps = [], [], []
    for k, sp in enumerate(specs):
        if sp is None:
            ims.append(None); arrs.append([]); bpps.append(32)
            continue
        im, a = _album(gpu, sp[0], sp[1], sp[2], sp[3], 6400 + 10 * k)
        ims.append(im); arrs.append(a); bpps.append(sp[4])
    outs, codes, launches = gpu.batch_download_fi(ims, bpps, fill=GUARD)
    bad = (1, 2, 4)
    assert [codes[i] for i in bad] == [gpu.IMP_ERROR_INVALID_ARGS] * 3, codes
    assert outs[1] == [] and all((o == GUARD).all() for i in (2, 4) for o in outs[i])
    good = [i for i in range(len(specs)) if i not in bad]
    _check(gpu, [ims[i] for i in good], [arrs[i] for i in good], [bpps[i] for i in good], [None] * len(good),
           [outs[i] for i in good], [codes[i] for i in good])
    # a pitch below the row refuses that handle alone as well
    outs, codes, _ = gpu.batch_download_fi([ims[0], ims[3]], [32, 24], [37 * 4 - 1, None], fill=GUARD)
    assert codes == [gpu.IMP_ERROR_INVALID_ARGS, 0] and all((o == GUARD).all() for o in outs[0])
    _check(gpu, [ims[3]], [arrs[3]], [24], [None], [outs[1]], [codes[1]])
    for im in ims:
        if im is not None:
            im.release()


def test_the_staging_cap_cuts_the_call_at_a_handle(gpu, monkeypatch):
    """Three albums of 375 KB of bitmaps each under a cap of 1 MB: the first two share a copy and a wait, the third goes in a
    group of its own -- the same bytes, a launch per group where the uncapped call makes one."""
    ims, arrs = [], []
    for k in range(3):
        a = [smooth_image(120, 160, 4, 6600 + 10 * k + f) for f in range(5)]
        ims.append(gpu.Image.album(a)); arrs.append(a)
    monkeypatch.setenv("IMPGPU_STAGE_CAP_MB", "1")
    outs, codes, launches = gpu.batch_download_fi(ims, [32] * 3, fill=GUARD)
    monkeypatch.delenv("IMPGPU_STAGE_CAP_MB")
    _check(gpu, ims, arrs, [32] * 3, [None] * 3, outs, codes)
    assert launches == 2, launches
    outs, codes, launches = gpu.batch_download_fi(ims, [32] * 3, fill=GUARD)
    assert codes == [0, 0, 0] and launches == 1, (codes, launches)
    for im in ims:
        im.release()


def test_frames_of_many_handles_behind_one_wait(gpu):
    ims, arrs = [], []
    for k, (c, frames, w, h) in enumerate([(4, 3, 37, 23), (3, 4, 33, 21), (4, 1, 45, 31), (1, 2, 50, 30), (3, 1, 41, 27), (4, 5, 64, 48)]):
        im, a = _album(gpu, c, frames, w, h, 6800 + 10 * k)
        ims.append(im); arrs.append(a)
    outs, codes = gpu.batch_album_download(ims[:3] + [None] + ims[3:])
    assert codes == [0, 0, 0, gpu.IMP_ERROR_INVALID_ARGS, 0, 0, 0] and outs[3] == []
    del outs[3]
    for i, (im, frames) in enumerate(zip(ims, arrs)):
        lone = im.frames()
        assert len(outs[i]) == len(lone) == len(frames), i
        for got, alone, a in zip(outs[i], lone, frames):
            assert np.array_equal(got, alone) and np.array_equal(got, a.reshape(got.shape)), i
    for im in ims:
        im.release()
