"""GIF answers past 256 colours written on the device (impgpu_album_encode_gif_ex / impgpu_batch_encode_gif_ex with
IMPGPU_GIF_ENC_QUANTIZE): k_gif_enc_claim, k_gif_enc_hist and k_gif_enc_cut between the colour sets and the tables, and the
cell -> index table in k_gif_enc_index.  The device's file must equal, byte for byte, gif_quant_model's -- written from
the definition's text -- and the host twin's; nothing at or behind out[length] may be written.  The shapes are the smallest
at which each part can still go wrong (gif_quant_model.CASES).  With flags = 0, and through the calls without _ex, the same
albums are refused as before, in the launches of before."""
import numpy as np
import pytest

import gif_quant_model as M
import test_gif_encode_host as E

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = 0, 1, 2, 50
LAUNCHES, LAUNCHES_PLAIN = 8, 5          # a group's launches under the flag (include/impgpu.h), and without it


def call_kw(kw):
    return dict(time_ms=kw.get("time_ms"), dispose=kw.get("dispose"), loop_count=kw.get("loop_count", -1), segment=kw.get("segment", 0))


def device_file(gpu, album, frames, kw):
    """the album under the flag: the model's file and the host twin's, and refused without the flag"""
    want = M.model_file_q(frames, **kw)
    rc, got, n, intact = gpu.encode_gif(album, flags=gpu.GIF_ENC_QUANTIZE, **kw)
    assert rc == OK and intact and n == len(want)
    assert got == want
    rc, host, n, intact = gpu.encode_gif_host(frames, flags=gpu.GIF_ENC_QUANTIZE, **kw)
    assert rc == OK and host == want
    for flags in (None, 0):
        rc, none, n, intact = gpu.encode_gif(album, flags=flags, **kw)
        assert rc == UNSUPPORTED and none is None and n == 0 and intact
    return got


def decodes_to_the_models_pixels(gpu, blob, frames):
    for flags in (0, gpu.GIF_SPLIT):
        rc, album = gpu.decode_gif(blob, 0, -1, flags=flags)
        assert rc == OK and album.count == len(frames) and album.shape == (frames[0].shape[0], frames[0].shape[1], 4)
        for f, b in zip(frames, album.frames()):
            if M.overflows(f):
                want, t = M.quantised_pixels(f)
            else:
                want, t = f[..., 2::-1], E.frame_keys(f)[1]
            assert np.array_equal(b[..., 2::-1][~t], want[~t])
            assert np.array_equal(b[..., 3] == 0, t) and (b[..., 3][~t] == 255).all()
        album.release()


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_file_is_the_models_and_the_host_twins(gpu, name):
    frames, kw = M.CASES[name]
    album = gpu.Image.album(frames)
    got = device_file(gpu, album, frames, kw)
    album.release()
    if name in ("noise_130x67", "noise_130x67_seg256", "album_exact_noise_holes"):
        decodes_to_the_models_pixels(gpu, got, frames)


def test_256_boundary_with_transparency(gpu):
    """255 colours and transparency fit: the flag changes nothing; 256 colours and transparency do not: K = 255"""
    rng = np.random.default_rng(4)
    exact = [E.frame_of(rng, 16, 16, E.palette(rng, 255), transparent=0.004)]
    assert not M.overflows(exact[0]) and E.frame_keys(exact[0])[1].any()
    album = gpu.Image.album(exact)
    plain = gpu.encode_gif(album)
    flagged = gpu.encode_gif(album, flags=gpu.GIF_ENC_QUANTIZE)
    assert plain[0] == OK and plain[1] == E.model_file(exact) and flagged == plain
    album.release()
    frames = M.CASES["bgra_256_and_holes"][0]
    assert len(M.quantise(frames[0])[0]) == 255


def test_a_view_with_padded_rows_at_odd_addresses(gpu):
    """130 x 67 noise as a window with step = 3 w + 5, at both segment sizes; the ramp with holes from an odd byte address"""
    frames = M.CASES["noise_130x67"][0]
    h, w, c = frames[0].shape
    step = 3 * w + 5
    raw = np.full((h * step + 3) & ~3, 0x5A, np.uint8)
    for y in range(h):
        raw[y * step: y * step + 3 * w] = frames[0][y].reshape(-1)
    carrier = gpu.Image(raw.reshape(1, -1, 1))
    view = gpu.Image.wrap(carrier.device_ptr, w, h, 3, step)
    for segment in (0, 256):
        device_file(gpu, view, frames, dict(segment=segment))
    view.release(); carrier.release()
    frames, kw = M.CASES["ramp_holes"]
    h, w, c = frames[0].shape
    raw = np.zeros(h * w * 4 + 4, np.uint8)
    raw[1: 1 + h * w * 4] = frames[0].reshape(-1)
    carrier = gpu.Image(raw.reshape(1, -1, 1))
    assert carrier.device_ptr % 4 == 0
    odd = gpu.Image.wrap(carrier.device_ptr + 1, w, h, 4, w * 4)
    device_file(gpu, odd, frames, kw)
    odd.release(); carrier.release()


def test_an_album_whose_union_fits_is_the_flagless_file(gpu):
    frames, kw = E.CASES["one_colour_3_frames"]
    album = gpu.Image.album(frames)
    plain = gpu.encode_gif(album, **kw)
    assert plain[0] == OK and plain[1] == E.model_file(frames, **kw)
    assert gpu.encode_gif(album, flags=gpu.GIF_ENC_QUANTIZE, **kw) == plain
    assert gpu.encode_gif(album, flags=0, **kw) == plain
    album.release()
    frames, kw = E.CASES["local_tables"]                                 # exact local tables stay exact local tables
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album, flags=gpu.GIF_ENC_QUANTIZE, **kw)
    assert rc == OK and intact and got == E.model_file(frames, **kw)
    album.release()


def test_a_batch_is_its_lone_calls_in_the_launches_of_one(gpu):
    rng = np.random.default_rng(8)
    sets = [
        ([np.zeros((9, 9, 1), np.uint8)], dict()),                                                  # refused: one channel
        ([E.frame_of(rng, 33, 21, E.palette(rng, 40), transparent=0.2)], dict(loop_count=0)),
        ([M.with_holes(rng, rng.integers(0, 256, (30, 40, 3)).astype(np.uint8), 0.2), E.frame_of(rng, 40, 30, E.palette(rng, 20))],
         dict(time_ms=[50, 60], dispose=[1, 2], loop_count=2)),
        (M.CASES["bgr_272"][0], dict()),
    ]
    Q = gpu.GIF_ENC_QUANTIZE
    albums = [gpu.Image.album(frames) for frames, _ in sets]
    lone = [gpu.encode_gif(a, flags=Q, segment=1024, **{k: v for k, v in call_kw(kw).items() if k != "segment"}) for a, (_, kw) in zip(albums, sets)]
    assert [r[0] for r in lone] == [UNSUPPORTED, OK, OK, OK]
    for (frames, kw), r in list(zip(sets, lone))[1:]:
        assert r[1] == M.model_file_q(frames, segment=1024, **kw)
    args = dict(time_ms=[kw.get("time_ms") for _, kw in sets], dispose=[kw.get("dispose") for _, kw in sets],
                loop_counts=[kw.get("loop_count", -1) for _, kw in sets], segment=1024)
    rc, results, launches = gpu.batch_encode_gif(albums, flags=Q, **args)
    assert rc == OK and launches == LAUNCHES
    assert [r[0] for r in results] == [UNSUPPORTED, OK, OK, OK] and all(r[3] for r in results)
    for k in range(4):
        assert results[k][1] == lone[k][1] and results[k][2] == lone[k][2]
    rc, res1, launches1 = gpu.batch_encode_gif([albums[1]], flags=Q)                               # only exact albums: the same launches
    assert rc == OK and res1[0][0] == OK and launches1 == LAUNCHES and res1[0][1] == E.model_file(sets[1][0])
    for flags in (None, 0):                                                                        # without the flag: as before
        rc, res0, launches0 = gpu.batch_encode_gif(albums, flags=flags, **args)
        assert rc == OK and launches0 == LAUNCHES_PLAIN
        assert [r[0] for r in res0] == [UNSUPPORTED, OK, UNSUPPORTED, UNSUPPORTED] and all(r[3] for r in res0)
        assert res0[1][1] == lone[1][1] and [r[2] for r in res0] == [0, lone[1][2], 0, 0]
    rc, res, launches = gpu.batch_encode_gif([albums[1]], flags=2)
    assert rc == INVALID_ARGS and launches == 0
    for a in albums:
        a.release()


def test_an_album_the_pool_has_no_room_for_goes_in_a_further_group(gpu, monkeypatch):
    """$IMPGPU_STAGE_CAP_MB = 1 leaves the pool one histogram slot: the album with two frames past 256 colours is deferred
    and encoded by the same call in a second group; the single frame beside it is not"""
    monkeypatch.setenv("IMPGPU_STAGE_CAP_MB", "1")
    sets = [M.CASES["album_exact_noise_holes"], M.CASES["bgr_272"]]
    albums = [gpu.Image.album(frames) for frames, _ in sets]
    rc, results, launches = gpu.batch_encode_gif(albums, time_ms=[kw.get("time_ms") for _, kw in sets], dispose=[kw.get("dispose") for _, kw in sets],
                                                 loop_counts=[kw.get("loop_count", -1) for _, kw in sets], segment=512, flags=gpu.GIF_ENC_QUANTIZE)
    assert rc == OK and launches == 2 * LAUNCHES
    for (frames, kw), r in zip(sets, results):
        assert r[0] == OK and r[3] and r[1] == M.model_file_q(frames, **dict(kw, segment=512))
    for a in albums:
        a.release()


@pytest.mark.parametrize("name", ["bgr_272", "album_exact_noise_holes"])
def test_capacity_one_byte_short(gpu, name):
    frames, kw = M.CASES[name]
    want = M.model_file_q(frames, **kw)
    album = gpu.Image.album(frames)
    rc, none, n, intact = gpu.encode_gif(album, flags=gpu.GIF_ENC_QUANTIZE, capacity=len(want) - 1, **kw)
    assert rc == MALLOC_FAILED and none is None and n == len(want) and intact
    rc, got, n, intact = gpu.encode_gif(album, flags=gpu.GIF_ENC_QUANTIZE, capacity=len(want), **kw)
    assert rc == OK and got == want and intact
    album.release()


def test_unknown_flags_are_refused(gpu):
    album = gpu.Image.album(M.CASES["bgr_272"][0])
    for flags in (2, 3, -1):
        rc, got, n, intact = gpu.encode_gif(album, flags=flags)
        assert rc == INVALID_ARGS and n == 0 and intact
    album.release()
