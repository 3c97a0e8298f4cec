"""IMPGPU_GIF_SPLIT on the device: impgpu_image_decode_gif_ex / impgpu_batch_decode_gif_ex cut every page at its clear codes
(k_gif_lzw_scan), measure every segment (k_gif_lzw_len) and decode every segment with a wavefront of its own
(k_gif_lzw_emit) in front of k_gif_compose_mix: four launches per call where the flag-less call makes two, the same
albums, codes and refusals file by file.  Every album must be what the flag-less call gives and what the oracle's LoadGIF
loop gives for the model's pages (tests/gif_writer.py); the pages made to be cut and the damage behind a cut are
test_gif_split_host.py's, whose model confirms the cuts.  Exact comparisons throughout."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gif_writer as G
import oracle_lib as orc
from conftest import ROOT
from test_gif_decode_host import rgb_table
from test_gif_split_host import cut_cases, damage_behind_a_cut, model_counts, noise, page_file
from test_gpu_gif_decode import bad_files, check_several_pieces, the_eight

pytestmark = pytest.mark.gpu


def oracle_frames(pages, destructive, pg):
    rc, frames = orc.gif_compose(pages, destructive, pg)
    assert rc == 0
    return frames


@pytest.fixture(scope="module")
def eight():
    sets = the_eight()
    return sets, [oracle_frames(pages, d, pg) for _, pages, d, pg in sets]


@pytest.fixture(scope="module")
def cuts():
    """the pages made to be cut: [(name, file, model pages, destructive, page)] and the oracle's albums"""
    sets = [(name, blob, G.parse(blob)[0], bool(i & 1), (-1, 0)[i % 2]) for i, (name, (blob, counts)) in enumerate(cut_cases().items())]
    assert sum(1 for name, blob, _, _, _ in sets if model_counts(blob)[0] > 1) >= 12
    return sets, [oracle_frames(pages, d, pg) for _, _, pages, d, pg in sets]


def same(albums, want, names):
    for name, album, w in zip(names, albums, want):
        got = album.frames()
        assert len(got) == len(w), name
        for f, (g, o) in enumerate(zip(got, w)):
            assert g.shape == o.shape and np.array_equal(g, o), (name, f)


def release(albums):
    for a in albums:
        if a is not None:
            a.release()


def test_the_eight_with_the_flag_four_launches_the_same_albums(gpu, eight):
    sets, want = eight
    files = [(b, d, p) for b, _, d, p in sets]
    rc, albums, codes, launches = gpu.batch_decode_gif(files, flags=gpu.GIF_SPLIT)
    assert rc == 0 and codes == [0] * 8 and launches == 4
    rc0, plain, codes0, launches0 = gpu.batch_decode_gif(files)
    assert rc0 == 0 and codes0 == [0] * 8 and launches0 == 2
    same(albums, want, range(8))
    same(plain, want, range(8))
    for i, (blob, pages, destructive, pg) in enumerate(sets):        # the lone _ex call equals the batch's entry
        rc1, alone = gpu.decode_gif(blob, destructive, pg, flags=gpu.GIF_SPLIT)
        assert rc1 == 0, i
        same([alone], [want[i]], [i])
        alone.release()
    release(albums + plain)


def test_pages_made_to_be_cut(gpu, cuts):
    sets, want = cuts
    names = [s[0] for s in sets]
    files = [(blob, d, pg) for _, blob, _, d, pg in sets]
    rc, albums, codes, launches = gpu.batch_decode_gif(files, flags=gpu.GIF_SPLIT)
    assert rc == 0 and codes == [0] * len(files) and launches == 4
    rc0, plain, codes0, launches0 = gpu.batch_decode_gif(files)
    assert rc0 == 0 and codes0 == [0] * len(files) and launches0 == 2
    same(albums, want, names)
    same(plain, want, names)
    for i in (0, 1, 5, 7, len(sets) - 1):
        rc1, alone = gpu.decode_gif(files[i][0], files[i][1], files[i][2], flags=gpu.GIF_SPLIT)
        assert rc1 == 0, names[i]
        same([alone], [want[i]], [names[i]])
        alone.release()
    release(albums + plain)


def test_twenty_segments_and_an_album_of_small_pages_in_one_call(gpu):
    big = page_file(noise(320, 240, 8), 8)
    assert model_counts(big) == [20]
    rng = np.random.default_rng(21)
    pages = [G.make_page(rng.integers(0, 16, (96, 96), dtype=np.uint8), palette=rgb_table(16, f), mcs=4, interlaced=bool(f & 1),
                         gce=dict(dispose=f % 4, key=(-1, 3)[f & 1], delay=f)) for f in range(8)]
    album = G.write(pages)
    assert model_counts(album) == [1] * 8
    files = [(big, False, -1), (album, False, -1)]
    want = [oracle_frames(G.parse(big)[0], False, -1), oracle_frames(G.model(pages), False, -1)]
    rc, albums, codes, launches = gpu.batch_decode_gif(files, flags=gpu.GIF_SPLIT)
    assert rc == 0 and codes == [0, 0] and launches == 4
    rc0, plain, codes0, launches0 = gpu.batch_decode_gif(files)
    assert rc0 == 0 and codes0 == [0, 0] and launches0 == 2
    same(albums, want, ["320x240", "album"])
    same(plain, want, ["320x240", "album"])
    release(albums + plain)


def test_a_call_that_leaves_in_several_pieces_with_the_flag(gpu):
    check_several_pieces(gpu, gpu.GIF_SPLIT, 4)


def test_damage_behind_a_cut_between_good_neighbours(gpu, eight, cuts):
    """Every bad file gets IMP_ERROR_DECODE_FAILED alone; the good albums of the same call, frames that lay in pool memory
    before it and a follow-up decode are what they were (every store goes through gif_store)."""
    sets, want = eight
    csets, cwant = cuts
    rng = np.random.default_rng(78)
    before = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for h, w in ((3, 5), (120, 130), (200, 200))]
    canaries = [gpu.Image(a) for a in before]
    bad = list(damage_behind_a_cut().items())
    good = [(sets[4][0], sets[4][2], sets[4][3], want[4]), (csets[0][1], csets[0][3], csets[0][4], cwant[0]),
            (csets[1][1], csets[1][3], csets[1][4], cwant[1]), (sets[7][0], sets[7][2], sets[7][3], want[7]),
            (csets[5][1], csets[5][3], csets[5][4], cwant[5]), (sets[0][0], sets[0][2], sets[0][3], want[0])]
    files, kinds = [], []
    for k, g in enumerate(good):
        files.append(g[:3]); kinds.append(k)
        if k < len(bad):
            files.append((bad[k][1][0], bool(k & 1), -1)); kinds.append(None)
    D = gpu.IMP_ERROR_DECODE_FAILED
    for flags, n in ((gpu.GIF_SPLIT, 4), (0, 2)):
        rc, albums, codes, launches = gpu.batch_decode_gif(files, flags=flags)
        assert rc == 0 and launches == n and codes == [0 if k is not None else D for k in kinds], flags
        for i, k in enumerate(kinds):
            if k is None:
                assert albums[i] is None, (flags, i)
            else:
                same([albums[i]], [good[k][3]], [(flags, i)])
        release(albums)
    for name, (blob, kind) in bad:                                     # the lone call says the same
        assert gpu.decode_gif(blob, flags=gpu.GIF_SPLIT)[0] == D, name
    for im, a in zip(canaries, before):
        assert np.array_equal(im.numpy(), a)
        im.release()
    rc, again, codes, launches = gpu.batch_decode_gif([g[:3] for g in good], flags=gpu.GIF_SPLIT)
    assert rc == 0 and codes == [0] * len(good) and launches == 4
    same(again, [g[3] for g in good], range(len(good)))
    release(again)


def test_refusals_page_requests_and_arguments(gpu, eight):
    sets, want = eight
    S = gpu.GIF_SPLIT
    bad = bad_files()
    mixed = [sets[1], bad[0], sets[2], bad[1], bad[2], bad[3], sets[4], bad[4], bad[5], sets[7]]
    files = [(m[0], False, -1) if len(m) == 2 else (m[0], m[2], m[3]) for m in mixed]
    rc, albums, codes, launches = gpu.batch_decode_gif(files, flags=S)
    assert rc == 0 and launches == 4 and codes == [0, 3, 0, 3, 3, 1, 0, 3, 3, 0]
    same([albums[i] for i in (0, 2, 6, 9)], [want[k] for k in (1, 2, 4, 7)], (0, 2, 6, 9))
    assert all(albums[i] is None for i in (1, 3, 4, 5, 7, 8))
    release(albums)
    for blob, code in bad:
        assert gpu.decode_gif(blob, flags=S)[0] == code
    # a page request: the pages behind it are neither decoded nor judged; `destructive` is the flag-less call's
    trailing = bad[2][0]
    rc, albums, codes, launches = gpu.batch_decode_gif([(trailing, False, 0), (trailing, False, 1), (trailing, True, -1), (trailing, False, 2)], flags=S)
    assert rc == 0 and codes == [0, 3, 3, 0] and launches == 4
    rc0, plain, codes0, _ = gpu.batch_decode_gif([(trailing, False, 0), (trailing, False, 2)])
    assert np.array_equal(albums[0].numpy(), plain[0].numpy()) and np.array_equal(albums[3].numpy(), plain[1].numpy())
    release(albums + plain)
    blob, pages = sets[7][0], sets[7][1]
    for destructive in (False, True):
        rc, a = gpu.decode_gif(blob, destructive, -1, flags=S)
        assert rc == 0
        same([a], [oracle_frames(pages, destructive, -1)], [destructive])
        a.release()
    # nothing accepted: nothing launched; count = 0, count = 257, a bad flag bit
    rc, albums, codes, launches = gpu.batch_decode_gif([(bad[3][0], False, -1), (sets[0][0], False, -2)], flags=S)
    assert rc == 0 and codes == [1, gpu.IMP_ERROR_INVALID_ARGS] and launches == 0 and albums == [None, None]
    rc, albums, codes, launches = gpu.batch_decode_gif([], flags=S)
    assert rc == 0 and launches == 0
    rc, albums, codes, launches = gpu.batch_decode_gif([], count=257, flags=S)
    assert rc == gpu.IMP_ERROR_INVALID_ARGS and launches == 0
    for flags in (2, 3, 4, -1, 1 << 30):
        rc, albums, codes, launches = gpu.batch_decode_gif([(sets[0][0], False, -1)], flags=flags)
        assert rc == gpu.IMP_ERROR_INVALID_ARGS and albums == [None] and launches == 0, flags
        assert gpu.decode_gif(sets[0][0], flags=flags)[0] == gpu.IMP_ERROR_INVALID_ARGS, flags
    assert gpu.lib.impgpu_batch_decode_gif_ex(None, None, None, None, 2, S, None, None, None) == gpu.IMP_ERROR_INVALID_ARGS
    assert gpu.lib.impgpu_image_decode_gif_ex(None, 0, 0, -1, S, None) == gpu.IMP_ERROR_INVALID_ARGS
    assert gpu.decode_gif(sets[0][0], False, -2, flags=S)[0] == gpu.IMP_ERROR_INVALID_ARGS


def test_without_an_env_a_bad_flag_is_refused_first_and_the_call_is_a_device_error():
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
import gif_writer as G
blob = G.write([G.make_page(np.zeros((2, 2), np.uint8), palette=np.zeros((4, 3), np.uint8), mcs=2)])
rc, albums, codes, launches = imp.batch_decode_gif([(blob, False, -1), (blob, True, 0)], flags=imp.GIF_SPLIT)
assert rc == imp.IMP_ERROR_DEVICE and codes == [imp.IMP_ERROR_DEVICE] * 2 and albums == [None, None] and launches == 0, (rc, codes, launches)
assert imp.decode_gif(blob, flags=imp.GIF_SPLIT)[0] == imp.IMP_ERROR_DEVICE
rc, albums, codes, launches = imp.batch_decode_gif([(blob, False, -1)], flags=2)      # before a device is looked for
assert rc == imp.IMP_ERROR_INVALID_ARGS and codes == [-1] and launches == 0, (rc, codes, launches)
assert imp.decode_gif(blob, flags=6)[0] == imp.IMP_ERROR_INVALID_ARGS
assert imp.gif_pages_split(blob) == (0, imp.gif_pages(blob, 0)[1], [1])                  # the host-only call needs none
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]


def test_a_split_album_feeds_the_operator_chain(gpu, eight):
    sets, _ = eight
    blob, pages, destructive, pg = sets[7]
    rc, decoded = gpu.decode_gif(blob, destructive, pg, flags=gpu.GIF_SPLIT)
    rc2, composed = gpu.gif_compose(pages, destructive, pg, album=True)
    assert rc == 0 and rc2 == 0 and decoded.count == composed.count == 40
    cfg = gpu.Config()
    res, _ = gpu.batch_run_ops([decoded, composed], [cfg, cfg], [dict(resize="32,0", simple=1)] * 2)
    assert [r[0] for r in res] == [0, 0] and decoded.shape == composed.shape and decoded.shape[1] == 32
    bitmaps, codes, _ = gpu.batch_download_fi([decoded, composed], [32, 32])
    assert codes == [0, 0] and len(bitmaps[0]) == len(bitmaps[1]) == 40
    for a, b in zip(bitmaps[0], bitmaps[1]):
        assert np.array_equal(a, b)
    assert len({a.tobytes() for a in bitmaps[0]}) > 1
    decoded.release(); composed.release(); cfg.release()


def test_a_call_past_the_staging_cap_is_cut_at_a_file_four_launches_per_group():
    """IMPGPU_STAGE_CAP_MB is read once per process: a child with a 1 MB cap decodes 24 files of 55 KB and 11 segments each --
    two groups, so eight launches with the flag and four without, the same albums."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import ngx_http_imgproc_amd as imp
from test_gif_split_host import model_counts, noise, page_file
blob = page_file(noise(200, 200, 8), 8)
assert model_counts(blob) == [11] and 24 * len(blob) > (1 << 20) > 12 * (len(blob) + 4096)
imp.env_start(0)
files = [(blob, bool(i & 1), -1) for i in range(24)]
rc, albums, codes, launches = imp.batch_decode_gif(files, flags=imp.GIF_SPLIT)
rc0, plain, codes0, launches0 = imp.batch_decode_gif(files)
assert rc == 0 and rc0 == 0 and codes == codes0 == [0] * 24, (codes, codes0)
first = plain[0].numpy()
for a, b in zip(albums, plain):
    assert np.array_equal(a.numpy(), first) and np.array_equal(b.numpy(), first)
    a.release(); b.release()
imp.env_destroy()
print("launches", launches, launches0)
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, IMPGPU_STAGE_CAP_MB="1"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.split()[-3:] == ["launches", "8", "4"], r.stdout
