"""GIF answers written on the device (impgpu_album_encode_gif / impgpu_batch_encode_gif): the five launches of
csrc/imp_gif_enc.hip on albums made with impgpu_album_upload.  The file must equal, byte for byte, test_gif_encode_host's
MODEL of the file's definition -- the model, never the library, says what the bytes are -- and nothing at or behind
out[length] may be written.  Every accepted file goes back through the device decoders (one wave per page, and cut at its
clear codes), which must return the source's colours and transparency; an album that went through the operator chain
encodes to the model of its downloaded frames; a batch gives what the lone calls give, in the launches of one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gif_writer as G
from conftest import ROOT
from test_gif_encode_host import CASES, INVALID_ARGS, MALLOC_FAILED, OK, UNSUPPORTED, frame_keys, frame_of, model_file, palette, refused_frames

pytestmark = pytest.mark.gpu


def round_trip(gpu, blob, frames):
    """the file through both decode routes (page by page, nothing carried from one page to the next): the frames' count
    and size, B,G,R where the source is not transparent, alpha 0 exactly where it is"""
    for flags in (0, gpu.GIF_SPLIT):
        rc, album = gpu.decode_gif(blob, 0, -1, flags=flags)
        assert rc == OK and album.count == len(frames) and album.shape == (frames[0].shape[0], frames[0].shape[1], 4)
        for f, b in zip(frames, album.frames()):
            _, t = frame_keys(f)
            assert np.array_equal(b[..., :3][~t], f[..., :3][~t])
            assert np.array_equal(b[..., 3] == 0, t) and (b[..., 3][~t] == 255).all()
        album.release()


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_is_the_models_and_decodes_to_the_source(gpu, name):
    frames, kw = CASES[name]
    want = model_file(frames, **kw)
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album, **kw)
    assert rc == OK and intact and n == len(want)
    assert got == want
    rc, again, n2, intact = gpu.encode_gif(album, capacity=n, **kw)                # an exact fit succeeds
    assert rc == OK and intact and again == want
    rc, none, n3, intact = gpu.encode_gif(album, capacity=n - 1, **kw)             # one byte short: the size, nothing written
    assert rc == MALLOC_FAILED and none is None and n3 == n and intact
    album.release()
    round_trip(gpu, got, frames)


def test_round_trip_of_an_animation_with_holes(gpu):
    rng = np.random.default_rng(11)
    pal = palette(rng, 90)
    frames = [frame_of(rng, 83, 47, pal[20 * i: 20 * i + 50], transparent=0.25 if i else 0.1) for i in range(3)]
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album, time_ms=[40, 50, 60], dispose=[1, 1, 1], loop_count=3, segment=300)
    assert rc == OK and intact and got == model_file(frames, time_ms=[40, 50, 60], dispose=[1, 1, 1], loop_count=3, segment=300)
    album.release()
    round_trip(gpu, got, frames)


def test_a_single_image_is_an_album_of_one(gpu):
    frames, kw = CASES["bgr_256"]
    im = gpu.Image(frames[0])
    rc, got, n, intact = gpu.encode_gif(im, **kw)
    assert rc == OK and intact and got == model_file(frames, **kw)
    im.release()


@pytest.mark.parametrize("name,frames", list(refused_frames()))
def test_too_many_colours_are_refused(gpu, name, frames):
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album)
    assert rc == UNSUPPORTED and got is None and n == 0 and intact
    album.release()


def test_argument_refusals(gpu):
    frames = CASES["one_colour_3_frames"][0]
    album = gpu.Image.album(frames)
    for segment in (-1, 1, 255, (1 << 24) + 1):
        assert gpu.encode_gif(album, segment=segment)[0] == INVALID_ARGS
    for dispose in ([0, 4, 0], [-1, 0, 0]):
        assert gpu.encode_gif(album, dispose=dispose)[0] == INVALID_ARGS
    assert gpu.encode_gif(album, loop_count=65536)[0] == INVALID_ARGS
    rc, got, n, intact = gpu.encode_gif(album, segment=1 << 24, loop_count=65535)
    assert rc == OK and intact and got == model_file(frames, segment=1 << 24, loop_count=65535)
    album.release()
    gray = gpu.Image(np.zeros((5, 7, 1), np.uint8))
    rc, got, n, intact = gpu.encode_gif(gray, capacity=4096)
    assert rc == UNSUPPORTED and n == 0 and intact
    gray.release()
    wide = gpu.Image(np.zeros((1, 4097, 3), np.uint8))
    rc, got, n, intact = gpu.encode_gif(wide, capacity=1 << 16)
    assert rc == UNSUPPORTED and n == 0 and intact
    wide.release()
    rc, results, launches = gpu.batch_encode_gif([], count=257)
    assert rc == INVALID_ARGS and launches == 0


def test_after_the_operators(gpu):
    """a decoded album through NN resize, a quarter turn and a pointwise filter keeps its colour count: the file is the
    model's of the frames the chain left"""
    rng = np.random.default_rng(5)
    rgb = palette(rng, 17)[:, ::-1]
    pages = [G.make_page(rng.integers(0, 17, (40, 50)).astype(np.uint8), mcs=5, gce=dict(dispose=1, delay=4 + i)) for i in range(3)]
    blob = G.write(pages, global_palette=np.concatenate([rgb, np.zeros((15, 3), np.uint8)]))
    rc, album = gpu.decode_gif(blob, 0, -1)
    assert rc == OK and album.count == 3 and album.shape == (40, 50, 4)
    cfg = gpu.Config()
    rc, step = gpu.run_ops(album, cfg, resize="25,0", simple=1, filters=["rotate=90", "modulate=60,70,80"])
    assert rc == OK and album.shape == (25, 20, 4)
    frames = album.frames()
    want = model_file(frames, time_ms=[40, 50, 60], dispose=[1, 1, 1], loop_count=0)
    assert want is not None and len(np.unique(np.concatenate([frame_keys(f)[0].reshape(-1) for f in frames]))) <= 17
    rc, got, n, intact = gpu.encode_gif(album, time_ms=[40, 50, 60], dispose=[1, 1, 1], loop_count=0)
    assert rc == OK and intact and got == want
    round_trip(gpu, got, frames)
    album.release(); cfg.release()


def test_a_batch_is_its_lone_calls_in_the_launches_of_one(gpu):
    rng = np.random.default_rng(3)
    p = palette(rng, 400)
    sets = [
        ([frame_of(rng, 33, 21, p[:40], transparent=0.2)], dict()),
        ([frame_of(rng, 70, 64, p[30 * i: 30 * i + 120], transparent=0.1) for i in range(4)], dict(time_ms=[10, 20, 30, 40], dispose=[1, 2, 3, 0], loop_count=2)),
        ([frame_of(rng, 20, 20, p[:257], alpha=False)], dict()),                                   # refused: 257 colours
        ([frame_of(rng, 129, 95, p[100:356], alpha=False) for _ in range(2)], dict(loop_count=0)),
        ([frame_of(rng, 5, 3, p[:7]) for _ in range(7)], dict(dispose=[1] * 7)),                  # capacity too small (below)
    ]
    albums = [gpu.Image.album(frames) for frames, _ in sets]
    lone = [gpu.encode_gif(a, time_ms=kw.get("time_ms"), dispose=kw.get("dispose"), loop_count=kw.get("loop_count", -1), segment=1024)
            for a, (_, kw) in zip(albums, sets)]
    assert [r[0] for r in lone] == [OK, OK, UNSUPPORTED, OK, OK]
    for (frames, kw), r in zip(sets, lone):
        assert r[1] == model_file(frames, segment=1024, **kw)
    caps = [None, None, None, None, lone[4][2] - 1]
    rc, results, launches = gpu.batch_encode_gif(albums, time_ms=[kw.get("time_ms") for _, kw in sets], dispose=[kw.get("dispose") for _, kw in sets],
                                                 loop_counts=[kw.get("loop_count", -1) for _, kw in sets], segment=1024, capacities=caps)
    assert rc == OK
    assert [r[0] for r in results] == [OK, OK, UNSUPPORTED, OK, MALLOC_FAILED]
    assert all(r[3] for r in results)                                                              # nothing behind a file, nothing for the refused
    for k in (0, 1, 3):
        assert results[k][1] == lone[k][1] and results[k][2] == lone[k][2]
    assert results[2][2] == 0 and results[4][2] == lone[4][2]
    one = gpu.Image.album([frame_of(rng, 9, 9, p[:5])])
    rc, res1, launches1 = gpu.batch_encode_gif([one])
    assert rc == OK and res1[0][0] == OK and launches == launches1 == 5
    rc, res0, launches0 = gpu.batch_encode_gif([albums[2]])                                        # refused on the device: still the launches
    assert rc == OK and res0[0][0] == UNSUPPORTED and launches0 == 5
    rc, res_none, launches_none = gpu.batch_encode_gif([])
    assert rc == OK and launches_none == 0
    for a in albums + [one]:
        a.release()


def test_many_segments_and_a_ragged_view(gpu):
    """1201 x 7 at segment 256: 33 segments whose cuts fall anywhere in a row; and a window of a wider BGR frame, whose
    rows are padded and start at odd addresses"""
    rng = np.random.default_rng(9)
    frames = [frame_of(rng, 1201, 7, palette(rng, 64), transparent=0.05)]
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album, segment=256)
    assert rc == OK and intact and got == model_file(frames, segment=256)
    album.release()
    big = frame_of(rng, 91, 40, palette(rng, 200), alpha=False)
    im = gpu.Image(big)
    cfg = gpu.Config()
    rc, step = gpu.run_ops(im, cfg, crop="61,33")
    assert rc == OK
    window = im.frames()
    rc, got, n, intact = gpu.encode_gif(im)
    assert rc == OK and intact and got == model_file(window)
    im.release(); cfg.release()


def test_no_env_no_device_is_looked_for():
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
rc, res, launches = imp.batch_encode_gif([None], segment=100)
assert rc == imp.IMP_ERROR_INVALID_ARGS and launches == 0, (rc, launches)
rc, res, launches = imp.batch_encode_gif([None])
assert rc == imp.IMP_ERROR_DEVICE and res[0][0] == imp.IMP_ERROR_DEVICE and launches == 0, (rc, res, launches)
f = np.zeros((3, 3, 3), np.uint8)
assert imp.encode_gif_host([f])[0] == 0
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]
