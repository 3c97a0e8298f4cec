"""GIF answers with delta frames, on the host (no GPU): impgpu_gif_encode_host_ex2 with IMPGPU_GIF_ENC_DELTA runs the lane
code csrc/imp_gif_enc.h adds for it -- the held rule, the window's bounds, the set of written keys, the choice, and index,
histogram and LZW through the window -- on one thread.  Its file must equal gif_delta_model's, byte for byte, which is
written from the definition's text (include/impgpu.h).  Pillow is the independent viewer: where no frame is quantised the
flagged file must composite to the canvases of the file without the bit, frame by frame, with the same frame count,
durations and loop.  Without the bit an _ex2 call is the _ex call."""
import io

import numpy as np
import pytest

import gif_writer as G
import gif_delta_model as D
import gif_quant_model as M
import test_gif_encode_host as E

import ngx_http_imgproc_amd as imp

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = 0, 1, 2, 50
Q = imp.GIF_ENC_QUANTIZE


def flags_of(quantize):
    return Q if quantize else None


def canvases(blob):
    """what Pillow shows: [(RGBA canvas, duration)], the loop count"""
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append((np.asarray(im.convert("RGBA")).copy(), im.info.get("duration", 0)))
    return out, im.info.get("loop", -1)


def pillow_sees_the_same(frames, kw, quantize=False):
    """The flagged file and the file without the bit composite to the same canvases in Pillow.  Pillow keeps the disposal
    method of the frame before where a frame says 0 ("unspecified": GifImagePlugin sets it only from non-zero bits), which
    GIF89a does not: so both files are made with 1 ("do not dispose") in place of 0.  The rule treats 0 and 1 alike, and the
    two flagged files may differ in the disposal bits alone."""
    dispose = kw.get("dispose")
    kw1 = dict(kw, dispose=[d or 1 for d in dispose]) if dispose else kw
    flagged = imp.encode_gif_host(frames, flags=flags_of(quantize), delta=True, **kw1)[1]
    asked = imp.encode_gif_host(frames, flags=flags_of(quantize), delta=True, **kw)[1]
    assert len(flagged) == len(asked) and sum(a != b for a, b in zip(flagged, asked)) == (list(dispose).count(0) if dispose else 0)
    plain = imp.encode_gif_host(frames, flags=flags_of(quantize), **kw1)[1]
    assert plain == E.model_file(frames, **kw1)
    same_canvases(flagged, plain)


def same_canvases(flagged, plain):
    a, loop_a = canvases(flagged)
    b, loop_b = canvases(plain)
    assert len(a) == len(b) and loop_a == loop_b
    for i, ((ca, da), (cb, db)) in enumerate(zip(a, b)):
        assert da == db, "frame %d: duration" % i
        assert np.array_equal(ca, cb), "frame %d: canvas" % i


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_file_is_the_models(name):
    frames, kw, quantize = D.CASES[name]
    want = D.model_file_d(frames, quantize=quantize, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, flags=flags_of(quantize), delta=True, **kw)
    assert rc == OK and intact and n == len(want)
    assert got == want
    assert n <= imp.gif_encode_bound(frames[0].shape[1], frames[0].shape[0], len(frames))
    pages, _ = G.parse(got)
    plan = D.plan(frames, kw.get("dispose"), quantize)
    assert [(p["left"], p["top"], p["width"], p["indices"].shape[0]) for p in pages] == [e["window"] for e in plan]
    if not any(e["quant"] for e in plan):
        rc, plain, n0, intact = imp.encode_gif_host(frames, flags=flags_of(quantize), **kw)
        assert rc == OK and plain == E.model_file(frames, **kw)
        pillow_sees_the_same(frames, kw, quantize)
        assert n <= n0 or not any(e["kind"] == "delta" for e in plan)


def test_cases_cover_what_they_claim():
    win = lambda name: [e["window"] for e in D.plan(D.CASES[name][0], D.CASES[name][1].get("dispose"), D.CASES[name][2])]
    kinds = lambda name: D.kinds(D.CASES[name][0], D.CASES[name][1].get("dispose"), D.CASES[name][2])
    assert win("identical_16x16") == [(0, 0, 16, 16), (0, 0, 1, 1)] and kinds("identical_16x16") == ["plain", "delta"]
    assert (D.plan(D.CASES["identical_16x16"][0])[1]["written"] == D.TRANSPARENT).all()
    assert [win("corner_" + c)[1] for c in ("top_left", "top_right", "bottom_left", "bottom_right")] == \
        [(0, 0, 1, 1), (15, 0, 1, 1), (0, 15, 1, 1), (15, 15, 1, 1)]
    w = win("bgra_130x67_seg256")
    assert w[1] == (7, 3, 114, 64) and w[2] == (7, 3, 114, 64)                # changes of items 0, 1 and 2 (rows 3, 40, 66) in one window
    assert 3 * 130 + 100 < 4096 <= 40 * 130 + 7 < 8192 <= 66 * 130 + 120
    assert 114 * 64 > 28 * 256 and -(-114 * 64 // 256) < -(-130 * 67 // 256)  # several segments live, planned ones idle
    assert kinds("bgr_3_channels") == ["plain", "delta", "delta"] and win("bgr_3_channels")[1:] == [(4, 2, 7, 3), (0, 0, 1, 1)]
    assert kinds("dispose_1200") == ["plain", "plain", "plain", "delta"]
    assert kinds("dispose_0311") == ["plain", "plain", "plain", "delta"]
    assert kinds("dispose_null") == ["plain", "delta", "delta", "delta"] and win("dispose_null")[2] == (0, 0, 20, 12)
    frames = D.CASES["transparent_over_opaque_and_back"][0]
    p = D.plan(frames)
    assert [e["window"] for e in p] == [(0, 0, 16, 16), (3, 2, 1, 1), (3, 2, 7, 8), (9, 9, 1, 1)]
    assert p[1]["written"][0, 0] == D.TRANSPARENT and p[2]["written"][0, 0] != D.TRANSPARENT and p[3]["written"][0, 0] == D.TRANSPARENT
    assert not D.held_mask(frames[1], frames[0])[2, 3] and not D.held_mask(frames[2], frames[1])[2, 3] and not D.held_mask(frames[3], frames[2])[9, 9]
    frames = D.CASES["exactly_256_plain"][0]
    wr = D.plan(frames)
    assert wr[1]["kind"] == "plain" and len(np.unique(D.keys_of(frames[1]))) == 256
    held = D.held_mask(frames[1], frames[0])
    assert D.window_of(held) == (0, 0, 17, 16) and held[0, 0] and len(np.unique(np.where(held, D.TRANSPARENT, D.keys_of(frames[1])))) == 257
    frames = D.CASES["exactly_255_delta"][0]
    wr = D.plan(frames)
    assert wr[1]["kind"] == "delta" and len(np.unique(D.keys_of(frames[1]))) == 255 and len(np.unique(wr[1]["written"])) == 256
    assert kinds("noise_over_held_border") == ["plain", "qdelta", "delta"]
    e = D.plan(D.CASES["noise_over_held_border"][0], None, True)[1]
    assert e["window"] == (6, 5, 28, 20) and (e["written"] == D.TRANSPARENT).sum() >= 1
    pages = D.model_pages_d(D.CASES["noise_over_held_border"][0], quantize=True)[0]
    assert [p["palette"].shape[0] for p in pages] == [8, 256, 2] and pages[1]["gce"]["key"] == 255


def test_exactly_256_colours_is_the_flagless_frame():
    frames, kw, _ = D.CASES["exactly_256_plain"]
    rc, got, n, intact = imp.encode_gif_host(frames, delta=True)
    assert rc == OK and got == imp.encode_gif_host(frames)[1] == E.model_file(frames)


def test_past_256_colours_without_quantize_is_refused_as_without_the_bit():
    frames, kw, quantize = D.CASES["noise_over_held_border"]
    assert quantize and D.model_file_d(frames, **kw) is None
    plain = imp.encode_gif_host(frames, flags=0, **kw)
    assert plain[0] == UNSUPPORTED
    assert imp.encode_gif_host(frames, delta=True, **kw) == plain
    assert imp.encode_gif_host(frames, flags=0, delta=True, **kw) == plain


def test_a_quantised_window_decodes_to_the_models_pixels():
    frames, kw, _ = D.CASES["noise_over_held_border"]
    got = imp.encode_gif_host(frames, flags=Q, delta=True, **kw)[1]
    pages, _ = G.parse(got)
    e = D.plan(frames, None, True)[1]
    want, t = M.quantised_pixels(D.as_bgra(e["written"]))
    p = pages[1]
    idx = p["indices"][::-1, :p["width"]]
    assert np.array_equal(idx == p["key"], t)
    assert np.array_equal(p["palette"][idx][..., 2::-1][~t], want[~t])


def test_strided_views():
    frames, kw, _ = D.CASES["bgra_130x67_seg256"]
    want = D.model_file_d(frames, **kw)
    h, w, c = frames[0].shape
    views = []
    for f in frames:
        wide = np.full((h, w + 5, c), 0x5A, np.uint8)
        wide[:, :w] = f
        views.append(wide[:, :w])
    assert views[0].strides[0] > w * c
    rc, got, n, intact = imp.encode_gif_host(views, delta=True, **kw)
    assert rc == OK and intact and got == want
    frames, kw, _ = D.CASES["bgr_3_channels"]                                   # 3-channel rows at odd addresses
    h, w, c = frames[0].shape
    views = []
    for f in frames:
        odd = np.zeros((h, w * 3 + 1), np.uint8)
        v = odd[:, : w * 3].reshape(h, w, 3)
        v[:] = f
        views.append(v)
    rc, got, n, intact = imp.encode_gif_host(views, delta=True, **kw)
    assert rc == OK and intact and got == D.model_file_d(frames, **kw)
    frames, kw, _ = D.CASES["transparent_over_opaque_and_back"]                 # 4-channel frames off the dword grid: the narrow read
    h, w, c = frames[0].shape
    views = []
    for f in frames:
        raw = np.zeros(h * w * 4 + 16, np.uint8)
        base = (-raw.ctypes.data) % 4 + 1
        v = raw[base: base + h * w * 4].reshape(h, w, 4)
        v[:] = f
        views.append(v)
    rc, got, n, intact = imp.encode_gif_host(views, delta=True, **kw)
    assert rc == OK and intact and got == D.model_file_d(frames, **kw)


@pytest.mark.parametrize("name", ["bgra_130x67_seg256", "noise_over_held_border"])
def test_capacity_one_byte_short(name):
    frames, kw, quantize = D.CASES[name]
    want = D.model_file_d(frames, quantize=quantize, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, flags=flags_of(quantize), delta=True, capacity=len(want) - 1, **kw)
    assert rc == MALLOC_FAILED and n == len(want) and intact
    rc, got, n, intact = imp.encode_gif_host(frames, flags=flags_of(quantize), delta=True, capacity=len(want), **kw)
    assert rc == OK and got == want and intact


def test_flag_bits(monkeypatch):
    frames, kw, _ = D.CASES["identical_16x16"]
    assert imp.GIF_ENC_DELTA == 2
    for flags in (4, 8, -1, 1 << 30):                                           # through _ex2: any bit but 1 and 2
        rc, got, n, intact = imp.encode_gif_host(frames, flags=flags, delta=True)
        assert rc == INVALID_ARGS and n == 0 and intact
    for flags in (2, 3):                                                        # the _ex call keeps refusing the bit
        assert imp.encode_gif_host(frames, flags=flags)[0] == INVALID_ARGS
    assert imp.encode_gif_host(frames, flags=Q, delta=True)[0] == OK            # both bits


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_without_the_bit_ex2_is_ex(name, monkeypatch):
    frames, kw, quantize = D.CASES[name]
    for flags in (0, Q):
        want = imp.encode_gif_host(frames, flags=flags, delta=False, **kw)
        assert want == imp.encode_gif_host(frames, flags=flags, **kw)
        monkeypatch.setattr(imp.ops, "GIF_ENC_DELTA", 0)                        # delta=True then calls _ex2 with `flags` alone
        assert imp.encode_gif_host(frames, flags=flags, delta=True, **kw) == want
        monkeypatch.undo()
        if want[0] == OK:
            assert want[1] == M.model_file_q(frames, **kw) if flags else want[1] == E.model_file(frames, **kw)


@pytest.mark.parametrize("name", sorted(E.CASES) + ["album_exact_noise_holes"])
def test_albums_of_the_earlier_cases(name):
    """the exact-palette and quantiser cases under the bit: dispose 2 and 3, holes, local tables, a quantised non-candidate"""
    frames, kw = E.CASES[name] if name in E.CASES else M.CASES[name]
    quantize = name not in E.CASES
    want = D.model_file_d(frames, quantize=quantize, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, flags=flags_of(quantize), delta=True, **kw)
    assert rc == OK and intact and got == want
    if not quantize:
        pillow_sees_the_same(frames, kw)
