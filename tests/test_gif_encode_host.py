"""GIF answers, on the host (no GPU): impgpu_gif_encode_host runs the lane code of the device encoder (csrc/imp_gif_enc.h:
colour sets, tables, index planes, the segmented LZW and the pack) on one thread.  Its file must equal, byte for byte, what
a MODEL of the file's definition (include/impgpu.h) gives: model_file() below -- np.unique for the colour sets,
np.searchsorted for the ranks, gif_writer's LZW encoder with clear codes at the segment cuts and gif_writer's container.
Pillow must open the file and find the frames, the loop count, the delays, the pixels and the transparency.  The model, the
frame makers and CASES are shared with the GPU test."""
import io
import struct

import numpy as np
import pytest

import gif_writer as G

import ngx_http_imgproc_amd as imp

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = 0, 1, 2, 50


# ---------------------------------------------------------------- the model of the file
def frame_keys(f):
    """(R << 16 | G << 8 | B per pixel, transparent mask) of a B,G,R[,A] frame"""
    f = np.asarray(f)
    rgb = (f[..., 2].astype(np.uint32) << 16) | (f[..., 1].astype(np.uint32) << 8) | f[..., 0].astype(np.uint32)
    t = (f[..., 3] == 0) if f.shape[2] == 4 else np.zeros(f.shape[:2], bool)
    return rgb, t


def model_table(colours, has_t):
    """sorted colours (+ the transparent entry) -> ((size, 3) R,G,B table, transparent index or -1, min_code_size)"""
    size = 2
    while size < len(colours) + has_t:
        size *= 2
    pal = np.zeros((size, 3), np.uint8)
    pal[: len(colours), 0] = colours >> 16
    pal[: len(colours), 1] = (colours >> 8) & 255
    pal[: len(colours), 2] = colours & 255
    return pal, (len(colours) if has_t else -1), max(2, size.bit_length() - 1)


def model_pages(frames, time_ms=None, dispose=None, segment=0):
    """-> (gif_writer pages, global palette or None), or None when the album is refused"""
    segment = segment or imp.GIF_ENC_SEGMENT
    h, w = frames[0].shape[:2]
    kt = [frame_keys(f) for f in frames]
    sets = [np.unique(k[~t]) for k, t in kt]
    ts = [bool(t.any()) for _, t in kt]
    union = np.unique(np.concatenate(sets))
    use_global = len(union) + any(ts) <= 256
    if not use_global and any(len(s) + t > 256 for s, t in zip(sets, ts)):
        return None
    pages = []
    for i, (k, t) in enumerate(kt):
        colours, has_t = (union, any(ts)) if use_global else (sets[i], ts[i])
        pal, tkey, mcs = model_table(colours, has_t)
        idx = np.searchsorted(colours, k).astype(np.int64)
        idx[t] = tkey
        gce = dict(dispose=dispose[i] if dispose else 0, key=tkey if ts[i] else -1, delay=min(65535, (time_ms[i] if time_ms else 0) // 10))
        pages.append(G.make_page(idx.astype(np.uint8), palette=None if use_global else pal, gce=gce, mcs=mcs,
                                 clear_at=range(segment, w * h, segment)))
    return pages, (model_table(union, any(ts))[0] if use_global else None)


def model_file(frames, time_ms=None, dispose=None, loop_count=-1, segment=0):
    """the file the encoders must write (loop counts other than 0 are patched into gif_writer's extension), or None"""
    m = model_pages(frames, time_ms, dispose, segment)
    if m is None:
        return None
    blob = bytearray(G.write(m[0], global_palette=m[1], loop=loop_count >= 0))
    if loop_count > 0:
        at = blob.index(b"NETSCAPE2.0") + 13
        blob[at:at + 2] = struct.pack("<H", loop_count)
    return bytes(blob)


# ---------------------------------------------------------------- frames
def palette(rng, n):
    """n distinct colours as (n, 3) B,G,R"""
    v = rng.choice(1 << 24, n, replace=False).astype(np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], 1).astype(np.uint8)


def frame_of(rng, w, h, colours, transparent=0.0, alpha=True):
    """a frame in which every colour of `colours` occurs; `transparent`: that share of pixels gets alpha 0 (and a colour of
    its own, which must not count)"""
    n = len(colours)
    pick = rng.integers(0, n, w * h)
    order = rng.permutation(w * h)
    pick[order[:n]] = np.arange(n)
    f = colours[pick].reshape(h, w, 3)
    if not alpha:
        return np.ascontiguousarray(f)
    a = rng.integers(1, 256, (h, w, 1)).astype(np.uint8)
    f = np.concatenate([f, a], 2)
    if transparent:
        hole = order[n:][: max(1, int(transparent * w * h))]              # never a colour's only pixel
        flat = f.reshape(-1, 4)
        flat[hole] = np.concatenate([rng.integers(0, 256, (len(hole), 3)), np.zeros((len(hole), 1))], 1).astype(np.uint8)
    return np.ascontiguousarray(f)


def make_cases():
    """name -> (frames, keyword arguments); the accepted albums of the issue's table"""
    rng = np.random.default_rng(20261020)
    cases = {}
    cases["one_colour_3_frames"] = ([np.full((5, 7, 3), (10, 200, 30), np.uint8) for _ in range(3)],
                                    dict(time_ms=[0, 95, 700000], dispose=[0, 1, 2], loop_count=0))
    cases["bgra_255_and_holes_seg256"] = ([frame_of(rng, 61, 59, palette(rng, 255), transparent=0.2)], dict(segment=256, dispose=[1]))
    cases["bgr_256"] = ([frame_of(rng, 64, 57, palette(rng, 256), alpha=False)], dict())
    p300 = palette(rng, 300)
    cases["local_tables"] = ([frame_of(rng, 40, 30, p300[50 * i: 50 * i + 200], transparent=0.1 if i == 1 else 0.0) for i in range(3)],
                             dict(time_ms=[100, 200, 300], dispose=[1, 1, 3], loop_count=0, segment=512))
    cases["noise_fills_table"] = ([palette(rng, 256)[rng.integers(0, 256, 96 * 64)].reshape(64, 96, 3).copy()], dict(segment=0))
    return cases


CASES = make_cases()


def refused_frames():
    rng = np.random.default_rng(7)
    yield "257_colours", [frame_of(rng, 20, 20, palette(rng, 257), alpha=False)]
    yield "256_colours_and_a_hole", [frame_of(rng, 20, 20, palette(rng, 256), transparent=0.01)]
    p = palette(rng, 400)
    yield "second_frame_257", [frame_of(rng, 20, 20, p[:100]), frame_of(rng, 20, 20, p[100:357])]


# ---------------------------------------------------------------- what Pillow must find
def check_with_pillow(blob, frames, time_ms=None, loop_count=-1):
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    assert im.format == "GIF" and im.size == (frames[0].shape[1], frames[0].shape[0])
    assert getattr(im, "n_frames", 1) == len(frames)
    assert im.info.get("loop", -1) == loop_count
    for i, f in enumerate(frames):
        im.seek(i)
        assert im.info.get("duration", 0) == min(65535, (time_ms[i] if time_ms else 0) // 10) * 10
        got = np.asarray(im.convert("RGBA"))
        _, t = frame_keys(f)
        assert np.array_equal(got[..., :3][~t], f[..., 2::-1][~t]), "frame %d: colours" % i
        if i == 0:
            assert np.array_equal(got[..., 3] == 0, t), "frame 0: transparency"


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_file_is_the_models(name):
    frames, kw = CASES[name]
    want = model_file(frames, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, **kw)
    assert rc == OK and intact and n == len(want)
    assert got == want
    assert n <= imp.gif_encode_bound(frames[0].shape[1], frames[0].shape[0], len(frames))
    pages, _ = G.parse(got)                                      # (gif_writer's own decoder reads it back, too)
    assert len(pages) == len(frames)
    check_with_pillow(got, frames, kw.get("time_ms"), kw.get("loop_count", -1))


def test_cases_cover_what_they_claim():
    frames, kw = CASES["one_colour_3_frames"]
    pages, gpal = model_pages(frames)
    assert gpal.shape == (2, 3) and pages[0]["mcs"] == 2
    frames, kw = CASES["bgra_255_and_holes_seg256"]
    pages, gpal = model_pages(frames, segment=256)
    assert gpal.shape == (256, 3) and pages[0]["gce"]["key"] == 255 and len(pages[0]["clear_at"]) == 14      # 15 segments, the last ragged
    assert 61 * 59 % 256 != 0
    pages, gpal = model_pages(CASES["local_tables"][0])
    assert gpal is None and all(p["palette"] is not None for p in pages)
    # the noise fills the 4096-entry table inside its one segment: with the deferred clear the stream is another one
    frames, kw = CASES["noise_fills_table"]
    pages, _ = model_pages(frames)
    idx = pages[0]["indices"].reshape(-1)
    assert len(idx) < imp.GIF_ENC_SEGMENT and pages[0]["clear_at"] == ()
    assert G.lzw_encode(idx, 8) != G.lzw_encode(idx, 8, never_clear=True)


@pytest.mark.parametrize("name,frames", list(refused_frames()))
def test_too_many_colours_are_refused(name, frames):
    assert model_file(frames) is None
    rc, got, n, intact = imp.encode_gif_host(frames)
    assert rc == UNSUPPORTED and n == 0 and intact


def test_rows_with_padding():
    frames, kw = CASES["bgra_255_and_holes_seg256"]
    h, w, c = frames[0].shape
    wide = np.full((h, w + 5, c), 0x5A, np.uint8)
    wide[:, :w] = frames[0]
    view = wide[:, :w]
    assert view.strides[0] > w * c
    rc, got, n, intact = imp.encode_gif_host([view], **kw)
    assert rc == OK and intact and got == model_file(frames, **kw)
    bgr = CASES["bgr_256"][0][0]                                   # a 3-channel frame whose rows start at odd addresses
    h, w = bgr.shape[:2]
    odd = np.zeros((h, w * 3 + 1), np.uint8)
    v3 = odd[:, : w * 3].reshape(h, w, 3)
    v3[:] = bgr
    rc, got, n, intact = imp.encode_gif_host([v3])
    assert rc == OK and intact and got == model_file([bgr])


@pytest.mark.parametrize("loop_count", [-1, 0, 5, 65535])
def test_loop_counts(loop_count):
    frames = CASES["one_colour_3_frames"][0]
    rc, got, n, intact = imp.encode_gif_host(frames, loop_count=loop_count)
    assert rc == OK and intact
    if loop_count <= 0:
        assert got == bytes(G.write(model_pages(frames)[0], global_palette=model_pages(frames)[1], loop=loop_count == 0))
    assert got == model_file(frames, loop_count=loop_count)
    check_with_pillow(got, frames, None, loop_count)


def test_single_transparent_frame_and_alpha_is_otherwise_ignored():
    f = np.zeros((4, 6, 4), np.uint8)
    f[..., :3] = (1, 2, 3)
    rc, got, n, intact = imp.encode_gif_host([f])                  # every pixel transparent: a table of the one entry
    assert rc == OK and got == model_file([f])
    g = f.copy()
    g[..., 3] = np.arange(1, 25).reshape(4, 6)                     # 24 alphas, one colour
    rc, got, n, intact = imp.encode_gif_host([g])
    assert rc == OK and got == model_file([g]) and len(G.parse(got)[0]) == 1


def test_argument_refusals():
    frames = CASES["one_colour_3_frames"][0]
    for segment in (-1, 1, 255, (1 << 24) + 1):
        assert imp.encode_gif_host(frames, segment=segment)[0] == INVALID_ARGS
    for segment in (256, 1 << 24):
        assert imp.encode_gif_host(frames, segment=segment)[0] == OK
    for dispose in ([0, 4, 0], [-1, 0, 0]):
        assert imp.encode_gif_host(frames, dispose=dispose)[0] == INVALID_ARGS
    assert imp.encode_gif_host(frames, loop_count=65536)[0] == INVALID_ARGS
    for c in (1, 2):
        rc, got, n, intact = imp.encode_gif_host([np.zeros((5, 7, c), np.uint8)])
        assert rc == UNSUPPORTED and n == 0 and intact
    assert imp.encode_gif_host([np.zeros((1, 4097, 3), np.uint8)])[0] == UNSUPPORTED
    assert imp.encode_gif_host([np.zeros((4097, 1, 3), np.uint8)])[0] == UNSUPPORTED
    assert imp.encode_gif_host([np.zeros((1, 4096, 3), np.uint8)])[0] == OK
    assert imp.encode_gif_host([np.zeros((1, 1, 3), np.uint8)] * 4097, capacity=1 << 20)[0] == UNSUPPORTED
    assert imp.gif_encode_bound(4097, 1, 1) == 0 and imp.gif_encode_bound(1, 1, 4097) == 0 and imp.gif_encode_bound(0, 1, 1) == 0


@pytest.mark.parametrize("name", ["bgra_255_and_holes_seg256", "local_tables"])
def test_capacity_one_byte_short(name):
    frames, kw = CASES[name]
    want = model_file(frames, **kw)
    rc, got, n, intact = imp.encode_gif_host(frames, capacity=len(want) - 1, **kw)
    assert rc == MALLOC_FAILED and n == len(want) and intact
    rc, got, n, intact = imp.encode_gif_host(frames, capacity=len(want), **kw)
    assert rc == OK and got == want and intact
