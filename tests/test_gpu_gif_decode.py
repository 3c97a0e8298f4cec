"""impgpu_image_decode_gif / impgpu_batch_decode_gif: GIF FILES in.  The host walks the container, k_gif_lzw decodes every
page of every file of the call on the device (one wavefront per page) into the index planes, k_gif_compose_mix follows:
two launches per call, one wait.  Every album must be what the oracle's LoadGIF loop (advancedio.c:204-247) gives for the
model's pages (tests/gif_writer.py, pinned against Pillow in test_gif_decode_host.py), what the lone call gives, and what
impgpu_gif_compose gives for those pages.  Exact comparisons throughout."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gif_writer as G
import oracle_lib as orc
from conftest import ROOT
from test_gif_decode_host import damaged_file, damaged_streams, rgb_table, single

pytestmark = pytest.mark.gpu


def edge_file(seed, cw, ch, n, mcs=4):
    """n pages on a cw x ch canvas whose rectangles hang over its right and bottom edges and touch the left and top ones
    (GIF offsets are unsigned), disposals 0..3 in turn, keys present and absent, local tables and the global one"""
    rng = np.random.default_rng(seed)
    spots = [(0, 0, cw, ch), (cw - 1, 0, 3, ch), (0, ch - 1, cw, 3), (1, 1, cw + 2, ch + 2), (0, 0, cw + 2, 2), (cw // 2, ch // 2, 1, 1), (0, 0, 2, ch + 3)]
    gpal = rgb_table(1 << mcs, seed)
    pages = []
    for f in range(n):
        left, top, w, h = spots[f % len(spots)]
        key = [-1, 0, 7, (1 << mcs) - 1][f % 4]
        idx = rng.integers(0, 1 << mcs, (h, w), dtype=np.uint8)
        idx[rng.random((h, w)) < 0.35] = max(key, 0)
        pages.append(G.make_page(idx, left, top, interlaced=bool(f & 1), palette=rgb_table(1 << mcs, seed + f) if f % 3 == 1 else None,
                                 gce=dict(dispose=f % 4, key=key, delay=f), mcs=mcs, block=(255, 7)[f & 1]))
    return G.write(pages, global_palette=gpal), G.model(pages, gpal)


def big_album(seed, n, cw, ch):
    """40 pages, mixed local tables, disposals 0..3, keys present and absent, rectangles anywhere on (and over) the canvas"""
    rng = np.random.default_rng(seed)
    gpal = rgb_table(256, seed)
    pages = []
    for f in range(n):
        if f == 0:
            w, h, left, top = cw, ch, 0, 0
        else:
            w, h = int(rng.integers(1, cw // 2)), int(rng.integers(1, ch // 2))
            left, top = int(rng.integers(0, cw)), int(rng.integers(0, ch))
        mcs = int(rng.integers(2, 9))
        key = int(rng.choice([-1, 0, 3])) if f % 3 else -1
        idx = (rng.integers(0, 1 << mcs, (h, w), dtype=np.uint8) if f % 2 else np.repeat(rng.integers(0, 1 << mcs, (h, 1), dtype=np.uint8), w, axis=1))
        pages.append(G.make_page(idx, left, top, interlaced=f % 5 == 2, palette=rgb_table(1 << mcs, seed + f) if f % 4 else None,
                                 gce=dict(dispose=f % 4, key=key, delay=f) if f % 7 else None, mcs=mcs, clear_at=(w * h // 2,) if f % 6 == 1 else ()))
    return G.write(pages, global_palette=gpal), G.model(pages, gpal)


def half_solid(w, h, mcs, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 1 << mcs, (h, w), dtype=np.uint8)
    idx[h // 4: h // 4 + 60] = 5
    p = G.make_page(idx, palette=rgb_table(1 << mcs, seed), mcs=mcs)
    return G.write([p]), G.model([p])


def the_eight():
    """(file, model pages, destructive, page)"""
    files = [
        single(1, 1, 2) + (-1,),
        edge_file(2, 3, 5, 7) + (6,),                                  # the last page
        single(64, 64, 2, interlaced=True) + (0,),
        single(257, 3, 7, clears=True) + (1,),                         # one past the last: page 0 (advancedio.c:114-116)
        half_solid(130, 120, 6, 5) + (-1,),
        single(200, 200, 8, never_clear=True, kind="solid") + (-1,),
        single(200, 200, 8, never_clear=True, kind="noise") + (0,),
        big_album(8, 40, 300, 200) + (-1,),
    ]
    return [(blob, pages, bool(i & 1), pg) for i, (blob, pages, pg) in enumerate(files)]


@pytest.fixture(scope="module")
def eight():
    sets = the_eight()
    want = []
    for blob, pages, destructive, pg in sets:
        rc, frames = orc.gif_compose(pages, destructive, pg)
        assert rc == 0
        want.append(frames)
    return sets, want


def test_eight_files_two_launches_equal_the_oracle_the_lone_call_and_the_compose_call(gpu, eight):
    sets, want = eight
    rc, albums, codes, launches = gpu.batch_decode_gif([(b, d, p) for b, _, d, p in sets])
    assert rc == 0 and codes == [0] * 8 and launches == 2
    for i, ((blob, pages, destructive, pg), w) in enumerate(zip(sets, want)):
        got = albums[i].frames()
        assert len(got) == len(w) == (1 if pg >= 0 else len(pages)), i
        rc1, alone = gpu.decode_gif(blob, destructive, pg)
        rc2, composed = gpu.gif_compose(pages, destructive, pg, album=True)
        assert rc1 == 0 and rc2 == 0, i
        for f, (g, o, a, c) in enumerate(zip(got, w, alone.frames(), composed.frames())):
            assert g.shape == o.shape and np.array_equal(g, o), (i, f)
            assert np.array_equal(g, a) and np.array_equal(g, c), (i, f)
        alone.release(); composed.release(); albums[i].release()


@functools.lru_cache(maxsize=None)
def several_pieces():
    """Five files of nine full-canvas 300 x 200 noise pages, and the oracle's albums: [(file, model pages, destructive, page)],
    [frames].  Noise does not compress, so a page's stream is longer than its 60 000 indices and the first four files put more
    than 2 MiB into the staging blob (asserted from the writer's streams): a piece of the buffer leaves before the last file
    has been copied in.  Nine streams are encoded; the files take them in turn, each page with a table, disposal and key of its own."""
    rng = np.random.default_rng(91)
    noise = [rng.integers(0, 256, (200, 300), dtype=np.uint8) for _ in range(9)]
    streams = [G.page_stream(G.make_page(idx, mcs=8)) for idx in noise]
    up16 = lambda v: (v + 15) & ~15
    files = []
    for i in range(5):
        pages = [G.make_page(noise[(f + i) % 9], palette=rgb_table(256, 40 + 9 * i + f), gce=dict(dispose=(f + i) % 4, key=(-1, 3, 255)[f % 3], delay=f),
                             mcs=8, lzw=streams[(f + i) % 9]) for f in range(9)]
        files.append((G.write(pages), G.model(pages), bool(i & 1), -1))
    entry = up16(9 * 48 + 9 * 8) + sum(1024 + up16(len(s)) for s in streams)
    assert min(len(s) for s in streams) > 60000 and 4 * entry > (2 << 20)
    want = []
    for blob, pages, destructive, pg in files:
        rc, frames = orc.gif_compose(pages, destructive, pg)
        assert rc == 0 and len(frames) == 9
        want.append(frames)
    return files, want


def check_several_pieces(gpu, flags, expect_launches):
    files, want = several_pieces()
    rc, albums, codes, launches = gpu.batch_decode_gif([(b, d, p) for b, _, d, p in files], flags=flags)
    assert rc == 0 and codes == [0] * 5 and launches == expect_launches
    for i, (blob, pages, destructive, pg) in enumerate(files):
        rc1, alone = gpu.decode_gif(blob, destructive, pg, flags=flags)
        got = albums[i].frames()
        assert rc1 == 0 and len(got) == 9, i
        for f, (g, o, a) in enumerate(zip(got, want[i], alone.frames())):
            assert g.shape == o.shape and np.array_equal(g, o) and np.array_equal(g, a), (i, f)
        alone.release()
        albums[i].release()


def test_a_call_that_leaves_in_several_pieces(gpu):
    check_several_pieces(gpu, 0, 2)


def bad_files():
    s = damaged_streams()
    return [
        (damaged_file(s["data that just stops"]), 3),
        (damaged_file(s["a code two above, later in the page"]), 3),
        (damaged_file(s["a whole extra string beyond the page"], trailing=True), 3),
        (b"\x89PNG\r\n\x1a\n" + bytes(64), 1),
        (damaged_file(s["a first code after a clear that is no literal"], trailing=True), 3),
        (damaged_file(s["indices beyond the page"]), 3),
    ]


def test_a_bad_file_gets_its_code_alone(gpu, eight):
    sets, want = eight
    bad = bad_files()
    mixed = [sets[1], bad[0], sets[2], bad[1], bad[2], bad[3], sets[4], bad[4], bad[5], sets[7]]
    files = [(m[0], False, -1) if len(m) == 2 else (m[0], m[2], m[3]) for m in mixed]
    rc, albums, codes, launches = gpu.batch_decode_gif(files)
    assert rc == 0 and launches == 2
    assert codes == [0, 3, 0, 3, 3, 1, 0, 3, 3, 0]
    for i, k in ((0, 1), (2, 2), (6, 4), (9, 7)):
        for g, o in zip(albums[i].frames(), want[k]):
            assert np.array_equal(g, o), i
        albums[i].release()
    assert all(albums[i] is None for i in (1, 3, 4, 5, 7, 8))
    for blob, code in bad:                                             # the lone call says the same
        assert gpu.decode_gif(blob)[0] == code
    # a damaged page BEHIND the requested one is neither decoded nor judged
    trailing = bad[2][0]
    rc, al = gpu.decode_gif(trailing, False, 0)
    rc_o, w = orc.gif_compose(G.parse(G.write([G.make_page(np.zeros((1, 1), np.uint8), palette=rgb_table(4, 1), mcs=2)]))[0], True, 0)
    assert rc == rc_o == 0 and np.array_equal(al.numpy(), w[0])
    al.release()
    rc, albums, codes, launches = gpu.batch_decode_gif([(trailing, False, 0), (trailing, False, 1), (trailing, True, -1), (trailing, False, 2)])
    assert rc == 0 and codes == [0, 3, 3, 0] and launches == 2         # (page 2 is past the end: page 0)
    albums[0].release(); albums[3].release()
    # nothing accepted: nothing launched
    rc, albums, codes, launches = gpu.batch_decode_gif([(bad[3][0], False, -1), (sets[0][0], False, -2)])
    assert rc == 0 and codes == [1, gpu.IMP_ERROR_INVALID_ARGS] and launches == 0 and albums == [None, None]


def test_damaged_neighbours_leave_everything_else_alone(gpu, eight):
    """The damaged streams end their pages with a status word and store nothing outside their planes: frames that lay in
    pool memory before the call, the good files' albums of the same call, and a follow-up decode are all what they were."""
    sets, want = eight
    rng = np.random.default_rng(77)
    before = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for h, w in ((3, 5), (64, 64), (120, 130), (200, 300))]
    canaries = [gpu.Image(a) for a in before]
    bad = bad_files()
    files = []
    for k in range(6):
        files += [(bad[k][0], bool(k & 1), -1), (sets[k][0], sets[k][2], sets[k][3])]
    rc, albums, codes, launches = gpu.batch_decode_gif(files)
    assert rc == 0 and launches == 2 and codes == [c for k in range(6) for c in (bad[k][1], 0)]
    for k in range(6):
        assert albums[2 * k] is None
        for g, o in zip(albums[2 * k + 1].frames(), want[k]):
            assert np.array_equal(g, o), k
    for im, a in zip(canaries, before):
        assert np.array_equal(im.numpy(), a)
        im.release()
    rc, again, codes, launches = gpu.batch_decode_gif([(s[0], s[2], s[3]) for s in sets[:6]])
    assert rc == 0 and codes == [0] * 6 and launches == 2
    for k in range(6):
        for g, o, first in zip(again[k].frames(), want[k], albums[2 * k + 1].frames()):
            assert np.array_equal(g, o) and np.array_equal(first, o), k
        again[k].release(); albums[2 * k + 1].release()


def test_arguments(gpu, eight):
    sets, _ = eight
    rc, albums, codes, launches = gpu.batch_decode_gif([])
    assert rc == 0 and launches == 0
    rc, albums, codes, launches = gpu.batch_decode_gif([], count=257)
    assert rc == gpu.IMP_ERROR_INVALID_ARGS and launches == 0
    assert gpu.lib.impgpu_batch_decode_gif(None, None, None, None, 2, None, None, None) == gpu.IMP_ERROR_INVALID_ARGS
    assert gpu.lib.impgpu_image_decode_gif(None, 0, 0, -1, None) == gpu.IMP_ERROR_INVALID_ARGS
    assert gpu.decode_gif(sets[0][0], False, -2)[0] == gpu.IMP_ERROR_INVALID_ARGS


def test_without_an_env_the_call_is_a_device_error():
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
import gif_writer as G
blob = G.write([G.make_page(np.zeros((2, 2), np.uint8), palette=np.zeros((4, 3), np.uint8), mcs=2)])
rc, albums, codes, launches = imp.batch_decode_gif([(blob, False, -1), (blob, True, 0)])
assert rc == imp.IMP_ERROR_DEVICE and codes == [imp.IMP_ERROR_DEVICE] * 2 and albums == [None, None] and launches == 0, (rc, codes, launches)
assert imp.decode_gif(blob)[0] == imp.IMP_ERROR_DEVICE
assert imp.gif_info(blob) == (0, (1, 2, 2)) and imp.gif_pages(blob, 1)[0] == 0      # the host-only calls need none
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]


def test_a_decoded_album_feeds_the_operator_chain(gpu, eight):
    """the decoded album and the composed album through impgpu_batch_run_ops (resize=32,0, simple) and the FI32 download"""
    sets, _ = eight
    blob, pages, destructive, pg = sets[7]
    rc, decoded = gpu.decode_gif(blob, destructive, pg)
    rc2, composed = gpu.gif_compose(pages, destructive, pg, album=True)
    assert rc == 0 and rc2 == 0 and decoded.count == composed.count == 40
    cfg = gpu.Config()
    res, _ = gpu.batch_run_ops([decoded, composed], [cfg, cfg], [dict(resize="32,0", simple=1)] * 2)
    assert [r[0] for r in res] == [0, 0] and decoded.shape == composed.shape and decoded.shape[1] == 32
    bitmaps, codes, _ = gpu.batch_download_fi([decoded, composed], [32, 32])
    assert codes == [0, 0] and len(bitmaps[0]) == len(bitmaps[1]) == 40
    for a, b in zip(bitmaps[0], bitmaps[1]):
        assert np.array_equal(a, b)
    assert len({a.tobytes() for a in bitmaps[0]}) > 1                  # (not forty copies of one frame)
    decoded.release(); composed.release(); cfg.release()
