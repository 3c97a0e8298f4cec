"""impgpu_png_info_ex / impgpu_png_scanlines_ex on the host (no GPU): the verdict for every colour type x depth x interlace
x tRNS combination and every PLTE rule; accept == 0 answers as the calls without _ex; the Adam7 layout of the filtered
stream, pass by pass, for every size from 1x1 to 17x17."""
import glob
import json
import os
import struct

import numpy as np
import pytest

import png_ext_writer as W

ROOT = os.path.dirname(os.path.abspath(__file__))
OK, UNSUP, DECODE = 0, 1, 3


@pytest.fixture(scope="module")
def imp():
    import ngx_http_imgproc_amd as imp

    return imp


def _samples(rng, colour, depth, w, h, top=None):
    return rng.integers(0, top or (1 << depth), size=(h, w, W.SPP[colour]), dtype=np.uint8)


def _want_verdict(colour, depth, interlace, trns, accept):
    """the mask rules of include/impgpu.h"""
    valid = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
    if depth not in valid[colour] or depth == 16 or colour == 4:
        return UNSUP
    if colour == 3:
        need = 1
        if trns:
            return UNSUP
    elif colour == 0 and depth < 8:
        need = 2
    else:
        need = 0
        if not interlace:
            return OK                                     # today's kinds
    if interlace:
        need |= 4
    return OK if (need & accept) == need else UNSUP


@pytest.mark.parametrize("accept", [0, 1, 2, 4, 7])
def test_info_ex_verdict_for_every_kind(imp, accept):
    rng = np.random.default_rng(5)
    for colour in (0, 2, 3, 4, 6):
        for depth in (1, 2, 4, 8, 16):
            for interlace in (0, 1):
                for trns in (False, True):
                    w, h = 13, 7
                    spp = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[colour]
                    bits = spp * depth
                    raw = b"".join(b"\x00" + bytes((w * bits + 7) // 8) for _ in range(h * 2))   # (enough bytes for any layout)
                    pal = rng.integers(0, 256, size=(min(1 << min(depth, 8), 256), 3), dtype=np.uint8) if colour == 3 else None
                    blob = W.write(np.zeros((h, w, 1), np.uint8), colour, depth, interlace, palette=pal,
                                   trns=b"\x00\x01" if trns else None, raw=raw)
                    rc, (gw, gh, gc) = imp.png_info_ex(blob, accept)
                    want = _want_verdict(colour, depth, interlace, trns, accept)
                    assert rc == want, (colour, depth, interlace, trns, accept, rc)
                    if rc == OK:
                        assert (gw, gh) == (w, h)
                        assert gc == {0: 1, 2: 3, 3: 3, 6: 4}[colour]
                    if accept == 0:
                        assert (rc, (gw, gh, gc) if rc == OK else None) == \
                               (imp.png_info(blob)[0], imp.png_info(blob)[1] if rc == OK else None)


def test_palette_plte_rules(imp):
    rng = np.random.default_rng(6)
    s = _samples(rng, 3, 4, 9, 5, top=3)
    pal = rng.integers(0, 256, size=(3, 3), dtype=np.uint8).tobytes()
    A = imp.PNG_PALETTE
    assert imp.png_info_ex(W.write(s, 3, 4, palette=pal), A) == (OK, (9, 5, 3))
    assert imp.png_info_ex(W.write(s, 3, 4), A)[0] == DECODE                            # no PLTE
    assert imp.png_info_ex(W.write(s, 3, 4, palette=b""), A)[0] == DECODE               # empty
    assert imp.png_info_ex(W.write(s, 3, 4, palette=pal[:7]), A)[0] == DECODE           # not a multiple of 3
    assert imp.png_info_ex(W.write(s, 3, 8, palette=bytes(771)), A)[0] == DECODE        # longer than 768 bytes
    assert imp.png_info_ex(W.write(s, 3, 8, palette=bytes(768)), A)[0] == OK            # 256 entries at depth 8
    assert imp.png_info_ex(W.write(s, 3, 4, palette=bytes(17 * 3)), A)[0] == UNSUP      # 17 entries > 2^4
    assert imp.png_info_ex(W.write(s, 3, 4, palette=bytes(16 * 3)), A)[0] == OK
    assert imp.png_info_ex(W.write(s, 3, 1, palette=bytes(3 * 3)), A)[0] == UNSUP       # 3 entries > 2^1
    two = W.write(s, 3, 4, palette=pal, extra=[W.chunk(b"PLTE", pal)])                 # two PLTE chunks
    assert imp.png_info_ex(two, A)[0] == DECODE
    late = W.write(s, 3, 4)                                                             # PLTE after the IDAT
    at = late.index(b"IEND") - 4
    late = late[:at] + W.chunk(b"PLTE", pal) + late[at:]
    assert imp.png_info_ex(late, A)[0] == DECODE
    crc = bytearray(W.write(s, 3, 4, palette=pal))                                      # PLTE's CRC damaged
    crc[crc.index(b"PLTE") + 4 + len(pal)] ^= 1
    assert imp.png_info_ex(bytes(crc), A)[0] == DECODE
    assert imp.png_info_ex(W.write(s, 3, 4, palette=pal, trns=b"\x00"), A)[0] == UNSUP
    # gray with a PLTE (a suggested palette, 11.2.3): not read
    g = _samples(rng, 0, 2, 9, 5)
    assert imp.png_info_ex(W.write(g, 0, 2, palette=b"\x01\x02"), imp.PNG_LOW_GRAY) == (OK, (9, 5, 1))


def test_size_limits_stay(imp):
    big_w = W.SIG + W.chunk(b"IHDR", struct.pack(">IIBBBBB", 4097, 4, 2, 3, 0, 0, 0)) + W.chunk(b"IEND", b"")
    big_h = W.SIG + W.chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 16385, 1, 0, 0, 0, 1)) + W.chunk(b"IEND", b"")
    assert imp.png_info_ex(big_w, imp.PNG_ALL)[0] == UNSUP
    assert imp.png_info_ex(big_h, imp.PNG_ALL)[0] == UNSUP


def test_accept_zero_is_the_old_calls_on_every_golden_png(imp):
    files = sorted(glob.glob(os.path.join(ROOT, "golden", "png", "*.png")))
    assert len(files) > 30
    for f in files:
        blob = open(f, "rb").read()
        assert imp.png_info_ex(blob, 0) == imp.png_info(blob), f
        want = imp.lib.impgpu_png_scanlines
        import ctypes as C

        n0, n1 = C.c_size_t(0), C.c_size_t(0)
        assert imp.lib.impgpu_png_scanlines_ex(blob, len(blob), 0, None, 0, C.byref(n1)) == want(blob, len(blob), None, 0, C.byref(n0))
        assert n0.value == n1.value
        rc0 = want(blob, len(blob), None, 0, C.byref(n0))
        if rc0 == imp.IMP_ERROR_MALLOC_FAILED:
            a, b = np.zeros(n0.value, np.uint8), np.zeros(n0.value, np.uint8)
            assert want(blob, len(blob), a.ctypes.data, a.size, C.byref(n0)) == \
                imp.lib.impgpu_png_scanlines_ex(blob, len(blob), 0, b.ctypes.data, b.size, C.byref(n1))
            assert np.array_equal(a, b)


def test_all_accepts_today_kinds_with_the_same_scanlines(imp):
    for f in sorted(glob.glob(os.path.join(ROOT, "golden", "png", "f_*.png"))):
        blob = open(f, "rb").read()
        assert imp.png_info_ex(blob, imp.PNG_ALL) == imp.png_info(blob), f
        assert imp.png_scanlines_ex(blob, imp.PNG_ALL) == imp.png_scanlines_ex(blob, 0), f


def test_adam7_layout_for_every_size_up_to_17(imp):
    """the filtered stream is the writer's, pass by pass, for every w x h in 1..17 (every pattern of empty passes), at
    depth 1 (several pixels per byte) and for RGB (three bytes per pixel)"""
    rng = np.random.default_rng(7)
    for w in range(1, 18):
        for h in range(1, 18):
            for colour, depth in ((0, 1), (2, 8)):
                s = _samples(rng, colour, depth, w, h)
                want = W.scanlines(s, colour, depth, 1, lambda p, j: (p + j) % 5)
                blob = W.write(s, colour, depth, 1, kinds=lambda p, j: (p + j) % 5)
                rc, got = imp.png_scanlines_ex(blob, imp.PNG_ALL)
                assert rc == OK and got == want, (w, h, colour)
                model_len = sum(ph * (1 + (pw * W.SPP[colour] * depth + 7) // 8) for _, _, _, _, _, pw, ph in W.passes(w, h, 1))
                assert len(got) == model_len


def test_damaged_streams_and_golden_verdicts(imp):
    man = json.load(open(os.path.join(ROOT, "golden", "png_ext", "manifest.json")))
    for name, m in man.items():
        blob = open(os.path.join(ROOT, "golden", "png_ext", name), "rb").read()
        rc, _ = imp.png_scanlines_ex(blob, imp.PNG_ALL)
        assert rc == m["code"], (name, rc)
    # n_interlaced.png: an Adam7 header over non-interlaced scanlines (444 bytes where Adam7 needs 455)
    blob = open(os.path.join(ROOT, "golden", "png", "n_interlaced.png"), "rb").read()
    assert imp.png_scanlines_ex(blob, imp.PNG_ALL)[0] == DECODE
    assert imp.png_scanlines_ex(blob, 0)[0] == UNSUP
    assert imp.png_info_ex(open(os.path.join(ROOT, "golden", "png", "n_palette.png"), "rb").read(), imp.PNG_ALL) == (OK, (12, 12, 3))
