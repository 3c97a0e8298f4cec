"""The GIF front's host side (no GPU): the container walk of include/impgpu_gif.h and the two host decoders behind
impgpu_gif_pages -- how = 0 a plain sequential LZW decoder, how = 1 the wave's rounds of csrc/imp_gif.h (the kernel's own
lane code) run one lane after the other.  tests/gif_writer.py is pinned against Pillow's decoder first; every comparison
is exact, pad bytes included."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import gif_writer as G
from conftest import ROOT

import ngx_http_imgproc_amd as imp

SHAPES = [(1, 1), (3, 5), (19, 37), (130, 120)]           # (w, h)


def rgb_table(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def single(w, h, mcs, interlaced=False, clears=False, never_clear=False, kind="noise", seed=0, block=255):
    """one full-screen page with a local table of 1 << mcs entries -> (file, model pages)"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h * 3 + mcs)
    if kind == "solid":
        idx = np.full((h, w), (1 << mcs) - 1, np.uint8)
    elif kind == "runs":                                   # long runs and noise mixed: long strings AND fresh literals
        idx = rng.integers(0, 1 << mcs, (h, w), dtype=np.uint8)
        idx[: h // 2] = idx[0, 0]
    else:
        idx = rng.integers(0, 1 << mcs, (h, w), dtype=np.uint8)
    n = w * h
    page = G.make_page(idx, interlaced=interlaced, palette=rgb_table(1 << mcs, seed + mcs), mcs=mcs,
                       clear_at=(n // 3, n // 2) if clears else (), never_clear=never_clear, block=block)
    return G.write([page]), G.model([page])


_cases = {}


def pin_cases():
    """every shape x code size x interlace x clears, and the 200 x 200 solid and noise pages that never clear"""
    if not _cases:
        for w, h in SHAPES:
            for mcs in range(2, 9):
                for interlaced in (False, True):
                    for clears in (False, True):
                        _cases["%dx%d_m%d_i%d_c%d" % (w, h, mcs, interlaced, clears)] = single(w, h, mcs, interlaced, clears, block=(255, 1, 17, 254)[mcs % 4])
        for kind in ("solid", "noise", "runs"):
            _cases["200x200_%s_never_clear" % kind] = single(200, 200, 8, never_clear=True, kind=kind)
        _cases["130x120_runs_interlaced_m5"] = single(130, 120, 5, True, True, kind="runs")
    return _cases


def test_the_writer_is_pinned_against_pillow():
    for name, (blob, pages) in pin_cases().items():
        got = np.asarray(Image.open(io.BytesIO(blob)))
        want = pages[0]["indices"][::-1, : pages[0]["width"]]
        assert got.shape == want.shape and np.array_equal(got, want), name
        parsed, canvas = G.parse(blob)                     # ... and the model's own parser and decoder against both
        assert np.array_equal(parsed[0]["indices"], pages[0]["indices"]) and np.array_equal(parsed[0]["palette"], pages[0]["palette"]), name


@pytest.mark.parametrize("how", [0, 1])
def test_gif_pages_equal_the_model_byte_for_byte(how):
    for name, (blob, pages) in pin_cases().items():
        rc, got = imp.gif_pages(blob, how)
        assert rc == 0 and got == G.planes(pages), (name, how)
        rc, (n, cw, ch) = imp.gif_info(blob)
        assert rc == 0 and (n, cw, ch) == (1, pages[0]["width"], pages[0]["indices"].shape[0]), name


def album_file(seed=5):
    """pages of many kinds in one file: offsets, local and global tables of 2..256 entries, code sizes, interlace, GCEs"""
    rng = np.random.default_rng(seed)
    gpal = rgb_table(64, seed)
    pages = []
    for f, (w, h, left, top, mcs, entries) in enumerate([(40, 30, 0, 0, 6, None), (7, 9, 3, 2, 2, 2), (40, 30, 0, 0, 8, 256), (33, 5, 5, 20, 4, 16),
                                                         (1, 1, 39, 29, 3, None), (17, 30, 23, 0, 5, 32)]):
        top_value = min(1 << mcs, entries or 64)
        idx = rng.integers(0, top_value, (h, w), dtype=np.uint8)
        gce = None if f == 2 else dict(dispose=f % 4, key=(f * 3) % top_value if f % 2 else -1, delay=f * 7)
        pages.append(G.make_page(idx, left, top, interlaced=bool(f & 1), palette=None if entries is None else rgb_table(entries, seed + f), gce=gce,
                                 mcs=mcs, clear_at=(w * h // 2,) if f % 3 == 0 else (), block=(255, 3, 100)[f % 3]))
    return G.write(pages, screen=(64, 48), global_palette=gpal, loop=True), G.model(pages, gpal)


@pytest.mark.parametrize("how", [0, 1])
def test_an_album_of_mixed_pages(how):
    blob, pages = album_file()
    rc, got = imp.gif_pages(blob, how)
    assert rc == 0 and got == G.planes(pages)
    assert imp.gif_info(blob) == (0, (6, 40, 30))          # the canvas is page 0, not the 64 x 48 logical screen
    parsed, canvas = G.parse(blob)
    assert canvas == (40, 30) and G.planes(parsed) == G.planes(pages)


# ---------------------------------------------------------------- impgpu_gif_walk itself, through a C99 shim
class Desc(C.Structure):
    _fields_ = [("left", C.c_int), ("top", C.c_int), ("width", C.c_int), ("height", C.c_int), ("interlaced", C.c_int), ("dispose", C.c_int),
                ("transparency_key", C.c_int), ("time_ms", C.c_int), ("palette_at", C.c_size_t), ("palette_entries", C.c_int),
                ("min_code_size", C.c_int), ("data_at", C.c_size_t), ("data_bytes", C.c_size_t)]


_shim = []


def walk(blob, cap=64):
    """impgpu_gif_walk -> (code, records, (canvas w, canvas h)); the header compiled as strict C99"""
    if not _shim:
        if shutil.which("gcc") is None:
            pytest.skip("needs gcc")
        out = os.path.join(ROOT, "tests", "c", "_build")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "gif_walk_shim.so")
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "c", "gif_walk_shim.c"), "-o", so])
        lib = C.CDLL(so)
        lib.gif_walk_shim.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Desc), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _shim.append(lib)
    recs = (Desc * max(1, cap))()
    n, cw, ch = C.c_int(), C.c_int(), C.c_int()
    rc = _shim[0].gif_walk_shim(bytes(blob), len(blob), recs, cap, n, cw, ch)
    return rc, [recs[i] for i in range(min(n.value, cap))], (cw.value, ch.value), n.value


def pillow_animation(seed, n, w, h, **kw):
    rng = np.random.default_rng(seed)
    frames = []
    base = rng.integers(0, 200, (h, w, 3), dtype=np.uint8)
    for f in range(n):
        a = base.copy()
        a[2 + f: 9 + f, 3 + 2 * f: 12 + 2 * f] = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)     # a moving patch: later pages are cropped
        frames.append(Image.fromarray(a).quantize(32 + 16 * f))
    buf = io.BytesIO()
    frames[0].save(buf, format="GIF", save_all=True, append_images=frames[1:], **kw)
    return buf.getvalue()


@pytest.mark.parametrize("seed,n,kw", [(1, 4, dict(duration=[30, 70, 110, 250], disposal=[0, 1, 2, 3], loop=0)),
                                       (2, 3, dict(duration=40, disposal=2, transparency=5, optimize=False))])
def test_walk_reports_real_pillow_animations_as_the_model_parser_does(seed, n, kw):
    blob = pillow_animation(seed, n, 48, 36, **kw)
    pages, canvas = G.parse(blob)
    rc, recs, got_canvas, count = walk(blob)
    assert rc == 0 and count == len(pages) and count > 1 and got_canvas == canvas
    for r, p in zip(recs, pages):
        assert (r.left, r.top, r.width, r.height) == (p["left"], p["top"], p["width"], p["indices"].shape[0])
        assert (r.dispose, r.transparency_key, r.time_ms) == (p["dispose"], p["key"], p["time_ms"])
    for how in (0, 1):                                      # and the pages Pillow's encoder wrote decode to the model's planes
        rc, got = imp.gif_pages(blob, how)
        assert rc == 0 and got == G.planes(pages)
    assert imp.gif_info(blob) == (0, (count,) + canvas)


def test_walk_records_name_tables_and_data():
    blob, pages = album_file()
    rc, recs, canvas, count = walk(blob)
    assert rc == 0 and count == 6 and canvas == (40, 30)
    assert [r.palette_entries for r in recs] == [64, 2, 256, 16, 64, 32]
    assert [r.min_code_size for r in recs] == [6, 2, 8, 4, 3, 5] and [r.interlaced for r in recs] == [0, 1, 0, 1, 0, 1]
    assert recs[0].palette_at == recs[4].palette_at == 13                    # the global table
    for r, p in zip(recs, pages):
        rgb = np.frombuffer(blob[r.palette_at: r.palette_at + 3 * r.palette_entries], np.uint8).reshape(-1, 3)
        assert np.array_equal(G.fi_palette(rgb), p["palette"])
        assert blob[r.data_at - 1] == r.min_code_size and r.data_bytes > 0
    assert recs[2].dispose == 0 and recs[2].transparency_key == -1 and recs[2].time_ms == 0     # no extension of its own
    rc, recs, canvas, count = walk(blob, cap=2)                              # too few records: the count still comes back
    assert rc == imp.IMP_ERROR_MALLOC_FAILED and count == 6 and len(recs) == 2


# ---------------------------------------------------------------- refusals and damage
def tiny(**kw):
    return G.make_page(np.zeros((1, 1), np.uint8), palette=rgb_table(4, 1), mcs=2, **kw)


def header_only_size(w, h):
    """a page whose descriptor says w x h over a stream of one pixel: the walk decompresses nothing"""
    p = G.make_page(np.zeros((1, 1), np.uint8), palette=rgb_table(4, 1), mcs=2)
    blob = bytearray(G.write([p]))
    at = blob.index(b"\x2c", 13)
    blob[at + 5: at + 9] = int(w).to_bytes(2, "little") + int(h).to_bytes(2, "little")
    return bytes(blob)


def test_refusals_are_unsupported():
    U = imp.IMP_ERROR_UNSUPPORTED
    good = G.write([tiny()])
    assert imp.gif_info(good)[0] == 0
    assert imp.gif_info(b"GIF88a" + good[6:])[0] == U and imp.gif_info(b"\x89PNG\r\n\x1a\n" + bytes(40))[0] == U and imp.gif_info(b"GIF")[0] == U
    no_table = G.make_page(np.zeros((2, 2), np.uint8), palette=None, mcs=2)
    assert imp.gif_info(G.write([no_table]))[0] == U
    assert imp.gif_info(G.write([no_table], global_palette=rgb_table(4, 2)))[0] == 0
    for mcs, want in ((1, U), (2, 0), (8, 0), (9, U), (0, U)):
        p = G.make_page(np.zeros((1, 1), np.uint8), palette=rgb_table(4, 1), mcs=mcs, lzw=b"\x44\x01")
        assert imp.gif_info(G.write([p]))[0] == want, mcs
    assert imp.gif_info(header_only_size(4096, 4096))[0] == 0
    assert imp.gif_info(header_only_size(4097, 1))[0] == U and imp.gif_info(header_only_size(1, 4097))[0] == U
    assert imp.gif_info(G.write([tiny()] * 4096))[:2] == (0, (4096, 1, 1))
    assert imp.gif_info(G.write([tiny()] * 4097))[0] == U
    empty = good[: good.index(b"\x2c", 13)] + b"\x3b"                        # no page at all
    assert imp.gif_info(empty)[0] == U
    for how in (0, 1):
        assert imp.gif_pages(G.write([no_table]), how)[0] == U
    assert imp.lib.impgpu_gif_pages(good, len(good), 2, None, 0, None) == imp.IMP_ERROR_INVALID_ARGS


def test_container_damage_is_decode_failed():
    D = imp.IMP_ERROR_DECODE_FAILED
    blob, _ = album_file()
    assert imp.gif_info(blob)[0] == 0
    for cut in range(6, len(blob)):                                           # every truncation: a chain past the end, or no trailer
        assert imp.gif_info(blob[:cut])[0] == D, cut
    assert imp.gif_info(G.write([tiny()], trailer=False))[0] == D
    assert imp.gif_info(header_only_size(0, 5))[0] == D and imp.gif_info(header_only_size(5, 0))[0] == D
    good = G.write([tiny()])
    at = good.index(b"\x2c", 13)
    assert imp.gif_info(good[:at] + b"\x99" + good[at + 1:])[0] == D          # an unknown block introducer
    long_block = bytearray(good)
    long_block[-5] = 200                                                  # the sub-block claims more than the file holds
    assert imp.gif_info(bytes(long_block))[0] == D
    for how in (0, 1):
        assert imp.gif_pages(blob[:-1], how)[0] == D


def bits(*codes):
    bw = G.BitWriter()
    for code, width in codes:
        bw.put(code, width)
    return bw.done()


def damaged_streams():
    """name -> a 3 x 2 page (mcs 2: clear 4, end 5, first free code 6) whose LZW stream is damaged in one stated way"""
    six = [1, 2, 3, 0, 1, 2]
    good = G.lzw_encode(six, 2)
    return {
        "a code above the next free code": bits((4, 3), (1, 3), (7, 3), (5, 3)),
        "a code two above, later in the page": bits((4, 3), (1, 3), (2, 3), (3, 3), (0, 4), (11, 4), (5, 4)),
        "a first code after a clear that is no literal": bits((4, 3), (6, 3), (5, 3)),
        "the same after a second clear": bits((4, 3), (1, 3), (4, 3), (7, 3), (5, 3)),
        "end of information too early": bits((4, 3), (1, 3), (2, 3), (5, 3)),
        "data that just stops": good[:2],
        "no data at all": b"",
        "indices beyond the page": G.lzw_encode(six + [3, 3, 3], 2),
        "a whole extra string beyond the page": G.lzw_encode(six * 3, 2),
    }


def damaged_file(stream, trailing=False):
    """the damaged page alone, or behind a good first page"""
    bad = G.make_page(np.zeros((2, 3), np.uint8), palette=rgb_table(4, 3), mcs=2, lzw=stream)
    return G.write(([tiny()] if trailing else []) + [bad])


@pytest.mark.parametrize("how", [0, 1])
def test_stream_damage_is_decode_failed(how):
    six = np.array([[1, 2, 3], [0, 1, 2]], np.uint8)
    ok = G.make_page(six, palette=rgb_table(4, 3), mcs=2)
    rc, got = imp.gif_pages(G.write([ok]), how)
    assert rc == 0 and got == G.planes(G.model([ok]))
    for name, stream in damaged_streams().items():
        for trailing in (False, True):
            blob = damaged_file(stream, trailing)
            assert imp.gif_info(blob)[0] == 0, name                           # the container is whole: only a decoder can tell
            assert imp.gif_pages(blob, how)[0] == imp.IMP_ERROR_DECODE_FAILED, (name, trailing)


def test_damage_never_writes_outside_the_planes():
    for name, stream in damaged_streams().items():
        blob = damaged_file(stream, True)
        n = C.c_size_t()
        assert imp.lib.impgpu_gif_pages(blob, len(blob), 0, None, 0, C.byref(n)) == imp.IMP_ERROR_MALLOC_FAILED and n.value == 4 + 8
        for how in (0, 1):
            buf = np.full(n.value + 64, 0xA5, np.uint8)
            assert imp.lib.impgpu_gif_pages(blob, len(blob), how, buf.ctypes.data, n.value, C.byref(n)) == imp.IMP_ERROR_DECODE_FAILED
            assert (buf[n.value:] == 0xA5).all(), name
