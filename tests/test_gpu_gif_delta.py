"""GIF answers with delta frames written on the device (impgpu_album_encode_gif_ex2 / impgpu_batch_encode_gif_ex2 with
IMPGPU_GIF_ENC_DELTA): k_gif_enc_delta ahead of the colour sets, and the DELTA instantiations of the launches behind it.
The device's file must equal, byte for byte, gif_delta_model's -- written from the definition's text -- and the host
twin's; nothing at or behind out[length] may be written.  The shapes are the smallest at which each part can still go wrong
(gif_delta_model.CASES).  Without the bit an _ex2 call is the _ex call, in bytes and launches."""
import numpy as np
import pytest

import gif_delta_model as D
import gif_quant_model as M
import test_gif_encode_host as E

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = 0, 1, 2, 50
LAUNCHES = {0: 5, 1: 8, 2: 6, 3: 9}      # a group's launches by flags (include/impgpu.h)


def flags_of(gpu, quantize):
    return gpu.GIF_ENC_QUANTIZE if quantize else None


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_file_is_the_models_and_the_host_twins(gpu, name):
    frames, kw, quantize = D.CASES[name]
    want = D.model_file_d(frames, quantize=quantize, **kw)
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album, flags=flags_of(gpu, quantize), delta=True, **kw)
    assert rc == OK and intact and n == len(want)
    assert got == want
    rc, host, n, intact = gpu.encode_gif_host(frames, flags=flags_of(gpu, quantize), delta=True, **kw)
    assert rc == OK and host == want
    rc, again, n2, intact = gpu.encode_gif(album, flags=flags_of(gpu, quantize), delta=True, capacity=len(want), **kw)
    assert rc == OK and intact and again == want
    rc, none, n3, intact = gpu.encode_gif(album, flags=flags_of(gpu, quantize), delta=True, capacity=len(want) - 1, **kw)
    assert rc == MALLOC_FAILED and none is None and n3 == len(want) and intact
    rc, res, launches = gpu.batch_encode_gif([album], time_ms=[kw.get("time_ms")], dispose=[kw.get("dispose")], loop_counts=[kw.get("loop_count", -1)],
                                             segment=kw.get("segment", 0), flags=flags_of(gpu, quantize), delta=True)
    assert rc == OK and res[0][:2] == (OK, want) and res[0][3] and launches == LAUNCHES[2 | (1 if quantize else 0)]
    if quantize:                                                        # without QUANTIZE: refused, with the code of the call without the bit
        plain = gpu.encode_gif(album, flags=0, **kw)
        assert plain[0] == UNSUPPORTED and gpu.encode_gif(album, delta=True, **kw) == plain
    album.release()


@pytest.mark.parametrize("name", ["bgra_130x67_seg256", "noise_over_held_border", "dispose_1200"])
def test_without_the_bit_ex2_is_ex(gpu, name, monkeypatch):
    frames, kw, quantize = D.CASES[name]
    album = gpu.Image.album(frames)
    args = dict(time_ms=[kw.get("time_ms")], dispose=[kw.get("dispose")], loop_counts=[kw.get("loop_count", -1)], segment=kw.get("segment", 0))
    for flags in (0, 1):
        lone = gpu.encode_gif(album, flags=flags, **kw)
        rc, res, launches = gpu.batch_encode_gif([album], flags=flags, **args)
        assert rc == OK and res[0] == lone and launches == LAUNCHES[flags]
        if lone[0] == OK:
            assert lone[1] == (M.model_file_q(frames, **kw) if flags else E.model_file(frames, **kw))
        monkeypatch.setattr(gpu.ops, "GIF_ENC_DELTA", 0)                # delta=True then calls _ex2 with `flags` alone
        assert gpu.encode_gif(album, flags=flags, delta=True, **kw) == lone
        rc2, res2, launches2 = gpu.batch_encode_gif([album], flags=flags, delta=True, **args)
        monkeypatch.undo()
        assert (rc2, res2, launches2) == (rc, res, launches)
    album.release()


def test_a_batch_is_its_lone_calls_in_the_launches_of_one(gpu):
    """one refused, one exact, one quantised, one with no candidate frame"""
    rng = np.random.default_rng(12)
    lonely = [E.frame_of(rng, 31, 17, E.palette(rng, 300)[100 * i: 100 * i + 120]) for i in range(3)]
    sets = [
        ([np.zeros((9, 9, 1), np.uint8)] * 2, dict()),                                              # refused: one channel
        (D.CASES["bgra_130x67_seg256"][0], dict(time_ms=[40, 50, 60], loop_count=0)),
        (D.CASES["noise_over_held_border"][0], dict(time_ms=[30, 30, 30])),
        (lonely, dict(dispose=[2, 3, 2], loop_count=1)),                                            # no candidate
    ]
    assert D.kinds(lonely, [2, 3, 2], True) == ["plain"] * 3
    Q = gpu.GIF_ENC_QUANTIZE
    albums = [gpu.Image.album(frames) for frames, _ in sets]
    lone = [gpu.encode_gif(a, flags=Q, delta=True, segment=256, **kw) for a, (_, kw) in zip(albums, sets)]
    assert [r[0] for r in lone] == [UNSUPPORTED, OK, OK, OK]
    for (frames, kw), r in list(zip(sets, lone))[1:]:
        assert r[1] == D.model_file_d(frames, segment=256, quantize=True, **kw)
    assert lone[3][1] == E.model_file(lonely, segment=256, **sets[3][1])
    args = dict(time_ms=[kw.get("time_ms") for _, kw in sets], dispose=[kw.get("dispose") for _, kw in sets],
                loop_counts=[kw.get("loop_count", -1) for _, kw in sets], segment=256)
    rc, results, launches = gpu.batch_encode_gif(albums, flags=Q, delta=True, **args)
    assert rc == OK and launches == LAUNCHES[3]
    assert [r[0] for r in results] == [UNSUPPORTED, OK, OK, OK] and all(r[3] for r in results)
    for k in range(4):
        assert results[k][1] == lone[k][1] and results[k][2] == lone[k][2]
    rc, results, launches = gpu.batch_encode_gif(albums, delta=True, **args)                        # without QUANTIZE: the noise is refused, alone
    assert rc == OK and launches == LAUNCHES[2]
    assert [r[0] for r in results] == [UNSUPPORTED, OK, UNSUPPORTED, OK] and all(r[3] for r in results)
    assert results[1][1] == lone[1][1] and results[3][1] == lone[3][1]
    rc, res, launches = gpu.batch_encode_gif([albums[1]], flags=4, delta=True)
    assert rc == INVALID_ARGS and launches == 0
    for flags in (4, 8, -1):
        rc, got, n, intact = gpu.encode_gif(albums[1], flags=flags, delta=True)
        assert rc == INVALID_ARGS and n == 0 and intact
    for flags in (2, 3):                                                                            # the _ex calls keep refusing the bit
        assert gpu.encode_gif(albums[1], flags=flags)[0] == INVALID_ARGS
    for a in albums:
        a.release()


def test_a_deferred_album_still_gets_its_lone_file(gpu, monkeypatch):
    """$IMPGPU_STAGE_CAP_MB = 1 leaves the pool one histogram slot: the album with two frames past 256 colours, one of them a
    quantised window, is deferred and encoded by the same call in a second group"""
    rng = np.random.default_rng(13)
    frames = [f.copy() for f in D.CASES["noise_over_held_border"][0]]
    frames[0][2:28, 3:37, :3] = rng.integers(0, 256, (26, 34, 3))                                   # frame 0 past 256 colours too: two slots
    assert D.kinds(frames, None, True) == ["qplain", "qdelta", "delta"]
    want = D.model_file_d(frames, segment=256, quantize=True)
    sets = [frames, M.CASES["bgr_272"][0]]
    monkeypatch.setenv("IMPGPU_STAGE_CAP_MB", "1")
    albums = [gpu.Image.album(f) for f in sets]
    rc, results, launches = gpu.batch_encode_gif(albums, segment=256, flags=gpu.GIF_ENC_QUANTIZE, delta=True)
    assert rc == OK and launches == 2 * LAUNCHES[3]
    assert results[0][0] == OK and results[0][3] and results[0][1] == want
    assert results[1][0] == OK and results[1][3] and results[1][1] == M.model_file_q(sets[1], segment=256)
    assert gpu.encode_gif(albums[0], segment=256, flags=gpu.GIF_ENC_QUANTIZE, delta=True)[1] == want
    for a in albums:
        a.release()


def test_a_flagged_file_decodes_to_the_written_windows(gpu):
    """page by page (nothing carried from one page to the next): inside a frame's window the written keys -- the colour, or
    alpha 0 where the pixel was held or transparent"""
    frames, kw, _ = D.CASES["bgra_130x67_seg256"]
    album = gpu.Image.album(frames)
    rc, got, n, intact = gpu.encode_gif(album, delta=True, **kw)
    assert rc == OK and intact
    album.release()
    plan = D.plan(frames)
    for flags in (0, gpu.GIF_SPLIT):
        rc, back = gpu.decode_gif(got, False, -1, flags=flags)
        assert rc == OK and back.count == len(frames) and back.shape == (67, 130, 4)
        for e, b in zip(plan, back.frames()):
            x0, y0, ww, wh = e["window"]
            win = b[y0:y0 + wh, x0:x0 + ww]
            t = e["written"] == D.TRANSPARENT
            assert np.array_equal(win[..., 3] == 0, t) and (win[..., 3][~t] == 255).all()
            assert np.array_equal(D.keys_of(win)[~t], e["written"][~t])
        back.release()
