"""impgpu_batch_gif_compose: many GIFs, one upload and ONE compose launch (k_gif_compose_mix) -- every album must be what
impgpu_gif_compose_album gives for that file alone and what the oracle gives (advancedio.c:204-247) -- and
impgpu_album_download_fi: IplToFI32 / IplToFI24 (advancedio.c:65-101) for every frame of an album behind one wait."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as orc
from conftest import ROOT, noise_image
from test_gif import page, palette, random_album

pytestmark = pytest.mark.gpu


def edge_album(seed, cw, ch, n):
    """Pages whose offsets hang over every edge of the canvas (left, top, right, bottom, all four), disposals 0..3 in turn,
    keys present and absent."""
    rng = np.random.default_rng(seed)
    spots = [(0, 0, cw, ch), (-2, 0, 3, ch), (0, -2, cw, 3), (cw - 1, 0, 3, ch), (0, ch - 1, cw, 3), (-1, -1, cw + 2, ch + 2)]
    pages = []
    for f in range(n):
        left, top, w, h = spots[f % len(spots)] if f else spots[0]
        key = [-1, 0, 7, 255][f % 4]
        idx = rng.integers(0, 256, (h, w), dtype=np.uint8)
        idx[rng.random((h, w)) < 0.35] = key if key >= 0 else 7
        pages.append(page(idx, left=left, top=top, dispose=f % 4, key=key, pal=palette(seed * 50 + f % 3), pad_value=int(rng.integers(1, 256))))
    return pages


# (pages, destructive, page): canvases 1x1, 3x5, 64x64, 257x3 (771 pixels: three 256-lane workgroups and three lanes of a
# fourth) and 300x200 with 40 pages; page = -1, 0, the last, one past the last
def the_eight():
    big = random_album(21, 40, 300, 200)
    return [
        (edge_album(1, 1, 1, 3), False, -1),
        (edge_album(2, 3, 5, 7), True, -1),
        (edge_album(3, 64, 64, 6), False, -1),
        (edge_album(4, 257, 3, 5), True, -1),
        (big, True, -1),
        (edge_album(5, 64, 64, 6), False, 0),
        (edge_album(6, 3, 5, 7), False, 6),           # the last page
        (edge_album(7, 257, 3, 5), True, 5),          # one past the last: page 0 (advancedio.c:114-116)
    ]


@pytest.fixture(scope="module")
def eight():
    sets = the_eight()
    want = []
    for pages, destructive, pg in sets:
        rc, frames = orc.gif_compose(pages, destructive, pg)
        assert rc == 0
        want.append(frames)
    return sets, want


def test_eight_sets_one_launch_equal_the_oracle_and_the_lone_call(gpu, eight):
    sets, want = eight
    rc, albums, codes, launches = gpu.batch_gif_compose(sets)
    assert rc == 0 and codes == [0] * 8 and launches == 1
    for i, ((pages, destructive, pg), w) in enumerate(zip(sets, want)):
        got = albums[i].frames()
        assert len(got) == len(w) == (1 if pg >= 0 else len(pages)), i
        rc1, alone = gpu.gif_compose(pages, destructive, pg, album=True)
        assert rc1 == 0
        for f, (g, o, a) in enumerate(zip(got, w, alone.frames())):
            assert g.shape == o.shape and np.array_equal(g, o), (i, f)
            assert np.array_equal(g, a), (i, f)
        alone.release()
        albums[i].release()


def test_a_bad_entry_gets_its_code_alone(gpu, eight):
    sets, want = eight
    broken = [dict(p) for p in sets[1][0]]
    broken[2]["width"] = broken[2]["indices"].shape[1] + 1            # pitch < width
    mixed = [sets[0], (sets[1][0], True, -2), sets[2], (None, False, -1), (broken, False, -1), sets[3]]
    rc, albums, codes, launches = gpu.batch_gif_compose(mixed)
    assert rc == 0 and codes == [0, gpu.IMP_ERROR_INVALID_ARGS, 0, gpu.IMP_ERROR_INVALID_ARGS, gpu.IMP_ERROR_INVALID_ARGS, 0] and launches == 1
    assert albums[1] is None and albums[3] is None and albums[4] is None
    for i, k in ((0, 0), (2, 2), (5, 3)):
        for g, o in zip(albums[i].frames(), want[k]):
            assert np.array_equal(g, o), i
        albums[i].release()
    # a broken page BEHIND the requested one is never walked: the lone call takes the set, so does the batch
    rc_l, alone = gpu.gif_compose(broken, False, 1, album=True)
    rc, albums, codes, launches = gpu.batch_gif_compose([(broken, False, 1)])
    assert rc_l == 0 and rc == 0 and codes == [0] and launches == 1 and np.array_equal(albums[0].numpy(), alone.numpy())
    alone.release(); albums[0].release()


def test_all_bad_launches_nothing_and_the_count_is_checked(gpu, eight):
    sets, _ = eight
    rc, albums, codes, launches = gpu.batch_gif_compose([(sets[0][0], False, -2), ([], False, -1)])
    assert rc == 0 and codes == [gpu.IMP_ERROR_INVALID_ARGS] * 2 and albums == [None, None] and launches == 0
    rc, albums, codes, launches = gpu.batch_gif_compose([])
    assert rc == 0 and launches == 0
    rc, albums, codes, launches = gpu.batch_gif_compose([], count=257)
    assert rc == gpu.IMP_ERROR_INVALID_ARGS and launches == 0
    assert gpu.lib.impgpu_batch_gif_compose(None, 2, None, None, None) == gpu.IMP_ERROR_INVALID_ARGS


def test_a_call_that_leaves_in_several_pieces(gpu):
    """Five albums of nine full-canvas 300 x 200 noise pages.  An entry is 512 + 9 * (1024 + 60 000) = 549 728 bytes of the
    blob, so the fourth ends 2 198 912 bytes behind the table -- past the 2 MiB at which a piece of the staging buffer leaves
    -- and the fifth is the last piece: one launch, every album the oracle's and the lone call's."""
    rng = np.random.default_rng(90)
    sets = [([page(rng.integers(0, 256, (200, 300), dtype=np.uint8), dispose=(f + i) % 4, key=(-1, 3, 255)[f % 3], pal=palette(900 + 10 * i + f % 2))
              for f in range(9)], bool(i & 1), -1) for i in range(5)]
    up16 = lambda v: (v + 15) & ~15
    entry = [up16(9 * 48 + 9 * 8) + sum(1024 + up16(p["indices"].size) for p in pages) for pages, _, _ in sets]
    assert entry == [549728] * 5 and sum(entry[:3]) < (2 << 20) < sum(entry[:4])
    rc, albums, codes, launches = gpu.batch_gif_compose(sets)
    assert rc == 0 and codes == [0] * 5 and launches == 1
    for i, (pages, destructive, pg) in enumerate(sets):
        rc_o, want = orc.gif_compose(pages, destructive, pg)
        rc1, alone = gpu.gif_compose(pages, destructive, pg, album=True)
        got = albums[i].frames()
        assert rc_o == 0 and rc1 == 0 and len(got) == len(want) == 9, i
        for f, (g, o, a) in enumerate(zip(got, want, alone.frames())):
            assert g.shape == o.shape and np.array_equal(g, o) and np.array_equal(g, a), (i, f)
        alone.release()
        albums[i].release()


def test_a_blob_past_the_staging_cap_is_cut_at_an_entry():
    """IMPGPU_STAGE_CAP_MB is read once per process: a child with a 1 MB cap composes four albums of 0.7 MB of pages each
    (no two fit one blob: a launch per entry) and an album that is past the cap by itself (alone, like its lone call)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import oracle_lib as orc, ngx_http_imgproc_amd as imp
from test_gif import page, palette
imp.env_start(0)
def full(seed, n):
    rng = np.random.default_rng(seed)
    return [page(rng.integers(0, 256, (200, 300), dtype=np.uint8), dispose=f %% 4, key=f %% 5, pal=palette(seed)) for f in range(n)]
sets = [(full(30 + i, 12), bool(i & 1), -1) for i in range(4)] + [(full(40, 30), True, -1)]
rc, albums, codes, launches = imp.batch_gif_compose(sets)
assert rc == 0 and codes == [0] * 5, codes
for (pages, d, p), al in zip(sets, albums):
    rc, want = orc.gif_compose(pages, d, p)
    assert rc == 0 and all(np.array_equal(g, w) for g, w in zip(al.frames(), want))
    al.release()
imp.env_destroy()
print("launches", launches)
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, IMPGPU_STAGE_CAP_MB="1"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.split()[-2:] == ["launches", "5"], r.stdout


@pytest.mark.parametrize("bpp", [24, 32])
def test_album_download_fi(gpu, bpp):
    frames = [noise_image(3, 5, 4, 60 + i) for i in range(3)]
    al = gpu.Image.album(frames)
    rc, got = al.frames_fi(bpp, fill=0xA5)
    assert rc == 0 and len(got) == 3
    tight = 5 * bpp // 8
    for g, f in zip(got, frames):
        want = orc.ipl_to_fi(f, bpp)
        assert g.shape == want.shape and np.array_equal(g[:, :tight], want[:, :tight])
        assert (g[:, tight:] == 0xA5).all()                            # the pitch padding is the caller's: left untouched
    # a wider pitch of the caller's own, and a single image as an album of one
    rc, got = al.frames_fi(bpp, pitch=tight + 7, fill=0x5A)
    assert rc == 0 and all(np.array_equal(g[:, :tight], orc.ipl_to_fi(f, bpp)[:, :tight]) and (g[:, tight:] == 0x5A).all() for g, f in zip(got, frames))
    al.release()
    bgr = noise_image(2, 6, 3, 70)
    im = gpu.Image(bgr)
    rc, got = im.frames_fi(bpp, fill=0xA5)
    want = orc.ipl_to_fi(bgr, bpp)
    tight = 6 * bpp // 8
    assert rc == 0 and len(got) == 1 and np.array_equal(got[0][:, :tight], want[:, :tight]) and (got[0][:, tight:] == 0xA5).all()
    assert im.frames_fi(16)[0] == gpu.IMP_ERROR_INVALID_ARGS and im.frames_fi(bpp, pitch=tight - 1)[0] == gpu.IMP_ERROR_INVALID_ARGS
    im.release()
    gray = gpu.Image(noise_image(2, 6, 1, 71))
    assert gray.frames_fi(bpp)[0] == gpu.IMP_ERROR_INVALID_ARGS
    gray.release()
