"""GIF answers past 256 colours, on the host (no GPU): impgpu_gif_encode_host_ex with IMPGPU_GIF_ENC_QUANTIZE and
impgpu_gif_quantize_host run the quantiser's lane code (csrc/imp_gif_enc.h: histogram, summed-volume table, cuts, colours,
cell -> index table) on one thread.  Their bytes must equal gif_quant_model's, which is written from the definition's text;
Pillow must decode each file to exactly the model's quantised pixels and transparency; without the flag the same inputs are
refused as before; and the definition itself must not be a degenerate one: on four inputs its error stays below Pillow's
FASTOCTREE."""
import io
import os

import numpy as np
import pytest

from conftest import ROOT
import gif_writer as G
import gif_quant_model as M
import test_gif_encode_host as E

import ngx_http_imgproc_amd as imp

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = 0, 1, 2, 50
Q = imp.GIF_ENC_QUANTIZE


def pillow_shows_the_models_pixels(blob, frames):
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    assert im.format == "GIF" and getattr(im, "n_frames", 1) == len(frames)
    for i, f in enumerate(frames):
        im.seek(i)
        got = np.asarray(im.convert("RGBA"))
        if M.overflows(f):
            want, t = M.quantised_pixels(f)
        else:
            want, t = f[..., 2::-1], E.frame_keys(f)[1]
        assert np.array_equal(got[..., :3][~t], want[~t]), "frame %d: colours" % i
        if i == 0:
            assert np.array_equal(got[..., 3] == 0, t), "frame 0: transparency"


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_file_is_the_models(name):
    frames, kw = M.CASES[name]
    assert any(M.overflows(f) for f in frames)
    want = M.model_file_q(frames, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, flags=Q, **kw)
    assert rc == OK and intact and n == len(want)
    assert got == want
    assert n <= imp.gif_encode_bound(frames[0].shape[1], frames[0].shape[0], len(frames))
    assert len(G.parse(got)[0]) == len(frames)
    pillow_shows_the_models_pixels(got, frames)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_quantize_host_is_the_models(name):
    frames, kw = M.CASES[name]
    for f in frames:                                               # (whatever the colour count: the exact frame of the album too)
        colours, T, idx = M.quantise(f)
        rc, table, tkey, indices = imp.gif_quantize_host(f)
        assert rc == OK and len(table) == len(colours) + T and tkey == (len(colours) if T else -1)
        assert np.array_equal(table[: len(colours)], M.model_table(colours, T)[0][: len(colours)])
        assert not T or tuple(table[-1]) == (0, 0, 0)
        assert np.array_equal(indices, idx)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_without_the_flag_nothing_changed(name):
    frames, kw = M.CASES[name]
    for flags in (None, 0):
        rc, got, n, intact = imp.encode_gif_host(frames, flags=flags, **kw)
        assert rc == UNSUPPORTED and got is None and n == 0 and intact


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_an_album_that_fits_gets_the_file_it_got(name):
    frames, kw = E.CASES[name]
    want = E.model_file(frames, **kw)
    assert M.model_file_q(frames, **kw) == want
    for flags in (0, Q):
        rc, got, n, intact = imp.encode_gif_host(frames, flags=flags, **kw)
        assert rc == OK and intact and got == want


def test_cases_cover_what_they_claim():
    sizes = lambda name: [(p["palette"].shape[0], p["mcs"], p["gce"]["key"]) for p in M.model_pages_q(*M.CASES[name][:1])[0]]
    assert sizes("bgr_272") == [(256, 8, -1)] and sizes("bgra_256_and_holes") == [(256, 8, 255)]
    assert len(M.quantise(M.CASES["bgra_256_and_holes"][0][0])[0]) == 255                 # K = 255 boxes and the transparent entry
    assert sizes("one_cell_400") == [(2, 2, -1)] and len(M.quantise(M.CASES["one_cell_400"][0][0])[0]) == 1
    assert sizes("two_cells_300") == [(2, 2, -1)] and len(M.quantise(M.CASES["two_cells_300"][0][0])[0]) == 2
    f = M.CASES["one_colour_and_296_rare"][0][0].reshape(-1, 3)
    u, counts = np.unique(f, axis=0, return_counts=True)
    assert len(u) == 297 and sorted(counts)[-2:] == [1, 3800]
    pages, gpal = M.model_pages_q(*M.CASES["album_exact_noise_holes"][:1])
    assert gpal is None and [p["palette"].shape[0] for p in pages] == [8, 256, 256] and [p["gce"]["key"] for p in pages] == [-1, -1, 255]
    assert 130 * 67 > imp.GIF_ENC_SEGMENT and 130 * 67 > 2 * 4096


def test_rows_with_padding_and_odd_addresses():
    frames, kw = M.CASES["noise_130x67"]
    h, w, c = frames[0].shape
    wide = np.full((h, 3 * w + 5), 0x5A, np.uint8)
    view = wide[:, : 3 * w].reshape(h, w, 3)
    view[:] = frames[0]
    assert view.strides[0] == 3 * w + 5
    rc, got, n, intact = imp.encode_gif_host([view], flags=Q, **kw)
    assert rc == OK and intact and got == M.model_file_q(frames, **kw)
    frames, kw = M.CASES["ramp_holes"]
    h, w, c = frames[0].shape
    want = M.model_file_q(frames, **kw)
    for offset in (0, 1):                                          # dword-aligned (the wide read) and not
        raw = np.zeros(h * w * 4 + 16, np.uint8)
        base = (-raw.ctypes.data) % 4 + offset
        v = raw[base: base + h * w * 4].reshape(h, w, 4)
        v[:] = frames[0]
        assert v.ctypes.data % 4 == offset
        rc, got, n, intact = imp.encode_gif_host([v], flags=Q, **kw)
        assert rc == OK and intact and got == want


@pytest.mark.parametrize("name", ["bgr_272", "album_exact_noise_holes"])
def test_capacity_one_byte_short(name):
    frames, kw = M.CASES[name]
    want = M.model_file_q(frames, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, flags=Q, capacity=len(want) - 1, **kw)
    assert rc == MALLOC_FAILED and n == len(want) and intact
    rc, got, n, intact = imp.encode_gif_host(frames, flags=Q, capacity=len(want), **kw)
    assert rc == OK and got == want and intact


def test_argument_refusals():
    frames = M.CASES["bgr_272"][0]
    for flags in (2, 3, -1, 1 << 30):
        rc, got, n, intact = imp.encode_gif_host(frames, flags=flags)
        assert rc == INVALID_ARGS and n == 0 and intact
    assert imp.encode_gif_host(frames, flags=Q, segment=255)[0] == INVALID_ARGS
    assert imp.encode_gif_host([np.zeros((5, 7, 1), np.uint8)], flags=Q)[0] == UNSUPPORTED
    assert imp.gif_quantize_host(np.zeros((5, 7, 1), np.uint8))[0] == UNSUPPORTED
    assert imp.gif_quantize_host(np.zeros((1, 4097, 3), np.uint8))[0] == UNSUPPORTED
    rc, table, tkey, indices = imp.gif_quantize_host(np.zeros((3, 4, 4), np.uint8))        # every pixel transparent: the one entry
    assert rc == OK and len(table) == 1 and tkey == 0 and not indices.any()


# ---------------------------------------------------------------- the definition is not a degenerate one
def quality_inputs():
    from PIL import Image

    for name in ("c420_q50_640x480.jpg", "c420_q92_opt_120x90.jpg"):
        yield name, np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "jpeg", name)).convert("RGB"))[..., ::-1].copy()
    yield "ramp", M.ramp()
    yield "noise", np.random.default_rng(1).integers(0, 256, (64, 64, 3)).astype(np.uint8)


@pytest.mark.parametrize("name,bgr", list(quality_inputs()))
def test_error_is_below_fastoctree(name, bgr):
    from PIL import Image

    rgb = np.ascontiguousarray(bgr[..., ::-1])
    mine, _ = M.quantised_pixels(bgr)
    theirs = np.asarray(Image.fromarray(rgb).quantize(256, method=Image.Quantize.FASTOCTREE, dither=Image.Dither.NONE).convert("RGB"))
    mse = lambda a: float(((a.astype(np.int64) - rgb.astype(np.int64)) ** 2).mean())
    print("%s: this definition %.1f, FASTOCTREE %.1f" % (name, mse(mine), mse(theirs)))
    assert mse(mine) < mse(theirs)
