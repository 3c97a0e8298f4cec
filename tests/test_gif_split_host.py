"""IMPGPU_GIF_SPLIT on the host (no GPU): impgpu_gif_pages_split runs the split route's three passes -- the scan that cuts
a page at its clear codes, the length pass and the emit pass of csrc/imp_gif.h, the kernels' own lane code -- one lane
after the other.  Its verdicts and planes must be impgpu_gif_pages(how = 0)'s, byte for byte, for good and damaged files,
and the number of segments must be what a MODEL of the cut rule says: segments_of() below, a table-free walk over
gif_writer.width_of.  The model, never the library, says how many segments a page has.  helpers: the page makers, the code
editor (read_codes / write_codes) and cut_cases() / damage_behind_a_cut() are shared with the sanitizer and GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gif_writer as G
from conftest import ROOT
from test_gif_decode_host import album_file, damaged_file, damaged_streams, header_only_size, pin_cases, rgb_table, tiny

import ngx_http_imgproc_amd as imp

MIN = imp.GIF_SPLIT_MIN_BYTES


# ---------------------------------------------------------------- the model of the cut rule
def read_codes(data, mcs):
    """the stream's codes as a decoder meets them, without a table: [(code, width, bit offset, codes since the last clear)],
    up to and including the code a decoder stops at for a reason visible without a table"""
    clear, end = 1 << mcs, (1 << mcs) + 1
    out, bit, nxt, since, first = [], 0, clear + 2, 0, True
    while True:
        w = G.width_of(nxt)
        if bit + w > len(data) * 8:
            return out
        c = (int.from_bytes(data[bit >> 3: (bit >> 3) + 3], "little") >> (bit & 7)) & ((1 << w) - 1)
        out.append((c, w, bit, since))
        bit += w
        since += 1
        if c == clear:
            nxt, since, first = clear + 2, 0, True
        elif c == end:
            return out
        elif first:
            if c >= clear:
                return out
            first = False
        else:
            if c > nxt or (c == nxt and nxt >= 4096):
                return out
            nxt = min(4096, nxt + 1)


def segments_of(data, mcs, min_bytes=None):
    """[(start bit, end bit or None for the open last one, the cutting clear's index in its stretch)]: a clear code is a cut
    when at least min_bytes of stream lie between the segment's start and the bit behind the clear, and the table of
    len(data) // min_bytes + 1 segments has room"""
    min_bytes = MIN if min_bytes is None else min_bytes
    cap = len(data) // min_bytes + 1
    segs, start = [], 0
    for c, w, bit, since in read_codes(data, mcs):
        if c == 1 << mcs and bit + w - start >= min_bytes * 8 and len(segs) + 2 <= cap:
            segs.append((start, bit + w, since))
            start = bit + w
    return segs + [(start, None, None)]


def write_codes(codes):
    bw = G.BitWriter()
    for c in codes:
        bw.put(c[0], c[1])
    return bw.done()


def streams(blob):
    """[(min_code_size, the sub-block payloads)] of a file's pages: a walk of the container that decodes nothing"""
    at = 13 + ((3 * (2 << (blob[10] & 7))) if blob[10] & 0x80 else 0)
    out = []
    while blob[at] != 0x3B:
        if blob[at] == 0x21:
            at += 2
            while blob[at]:
                at += blob[at] + 1
            at += 1
            continue
        assert blob[at] == 0x2C
        f = blob[at + 9]
        at += 10 + ((3 * (2 << (f & 7))) if f & 0x80 else 0)
        mcs = blob[at]
        at += 1
        data = bytearray()
        while blob[at]:
            data += blob[at + 1: at + 1 + blob[at]]
            at += blob[at] + 1
        at += 1
        out.append((mcs, bytes(data)))
    return out


def model_counts(blob):
    return [len(segments_of(data, mcs)) for mcs, data in streams(blob)]


# ---------------------------------------------------------------- the library's two answers, damaged files included
def raw(blob, split):
    """-> (code, the planes' bytes whatever the code or None when they were not written, segments or None)"""
    blob = bytes(blob)
    n = C.c_size_t(0)
    if split:
        rc = imp.lib.impgpu_gif_pages_split(blob, len(blob), None, 0, C.byref(n), None, 0)
    else:
        rc = imp.lib.impgpu_gif_pages(blob, len(blob), 0, None, 0, C.byref(n))
    if rc != imp.IMP_ERROR_MALLOC_FAILED:
        return rc, None, None
    pages = imp.gif_info(blob)[1][0]
    frame = np.full(n.value + 128, 0xA5, np.uint8)          # the planes in a buffer of exactly their size inside a guard frame
    segs = (C.c_int * pages)(*([-7] * pages))
    if split:
        rc = imp.lib.impgpu_gif_pages_split(blob, len(blob), frame[64:].ctypes.data, n.value, C.byref(n), segs, pages)
    else:
        rc = imp.lib.impgpu_gif_pages(blob, len(blob), 0, frame[64:].ctypes.data, n.value, C.byref(n))
    assert (frame[:64] == 0xA5).all() and (frame[64 + n.value:] == 0xA5).all()
    return rc, frame[64: 64 + n.value].tobytes(), list(segs) if split else None


def same_as_the_plain_decoder(blob, name, counts=None):
    rc0, planes0, _ = raw(blob, False)
    rc, planes, segs = raw(blob, True)
    assert rc == rc0 and planes == planes0, name
    if planes is not None:
        assert segs == (model_counts(blob) if counts is None else counts), name
    wrc, wplanes, wsegs = imp.gif_pages_split(blob)        # the Python mirror says the same
    assert wrc == rc and wsegs == segs and wplanes == (planes if rc == 0 else None), name
    return rc, segs


# ---------------------------------------------------------------- pages made to be cut
def page_file(idx, mcs, **kw):
    page = G.make_page(idx, palette=rgb_table(1 << mcs, mcs), mcs=mcs, **kw)
    return G.write([page])


def noise(w, h, mcs, seed=1):
    return np.random.default_rng(seed * 977 + w * 7 + h * 3 + mcs).integers(0, 1 << mcs, (h, w), dtype=np.uint8)


def runs(w, h, mcs, seed=1):
    a = noise(w, h, mcs, seed)
    a[: h // 2] = a[0, 0]
    return a


def clear_in_round(idx, mcs, want, lo):
    """a pixel position for clear_at such that the clear written there is code `want` of its stretch (the model says so)
    and a cut; searched from pixel `lo` on"""
    px = idx.reshape(-1)
    for at in range(lo, len(px) - 1):
        data = G.lzw_encode(px, mcs, clear_at=(at,))
        cuts = segments_of(data, mcs)[:-1]
        if cuts and cuts[0][2] == want:
            return at, data
        assert not cuts or cuts[0][2] < want, "the search ran past the round"
    raise AssertionError("no such position")


_cut = {}


def cut_cases():
    """name -> (file, segments per page as the model counts them)"""
    if _cut:
        return _cut
    c = {}
    c["130x120_noise_m8"] = page_file(noise(130, 120, 8), 8)
    c["200x200_noise_m8"] = page_file(noise(200, 200, 8), 8)
    c["200x200_noise_never_clear"] = page_file(noise(200, 200, 8), 8, never_clear=True)
    c["200x200_noise_m2"] = page_file(noise(200, 200, 2), 2)
    c["200x200_noise_m4"] = page_file(noise(200, 200, 4), 4)
    c["130x120_noise_m8_interlaced"] = page_file(noise(130, 120, 8), 8, interlaced=True)
    c["131x75_noise_m6_interlaced"] = page_file(noise(131, 75, 6), 6, interlaced=True)
    c["130x120_noise_m8_clear_every_1000"] = page_file(noise(130, 120, 8), 8, clear_at=range(1000, 15600, 1000))
    c["200x200_runs_m8"] = page_file(runs(200, 200, 8), 8)
    # the cutting clear as code 0, 1 and 63 of a round, and code 0 of the round after: a stretch's rounds are 64 codes each
    a = noise(64, 48, 8, 3)
    first = -(-(MIN * 8) // (9 * 64))                      # the first round that lies wholly behind MIN bytes of 9..12-bit codes
    lo = 64 * first - 8
    for want in (64 * first, 64 * first + 1, 64 * first + 63, 64 * first + 64):
        at, data = clear_in_round(a, 8, want, lo)
        lo = at
        c["64x48_clear_as_code_%d_of_its_round_%d" % (want % 64, want // 64)] = page_file(a, 8, lzw=data)
    # two clears in a row at a cut; a clear directly followed by EOI; a cutting clear as the very last code
    px = noise(130, 120, 8).reshape(-1)
    data = G.lzw_encode(px, 8)
    codes = read_codes(data, 8)
    behind = segments_of(data, 8)[0][1]
    cut = [k for k, (code, w, bit, since) in enumerate(codes) if bit + w == behind][0]
    c["130x120_two_clears_at_a_cut"] = page_file(px.reshape(120, 130), 8, lzw=write_codes(codes[: cut + 1] + [(256, 9)] + codes[cut + 1:]))
    short = noise(60, 50, 8, 5)                            # 3000 pixels: one stretch of more than MIN bytes, the table not yet full
    codes = read_codes(G.lzw_encode(short.reshape(-1), 8), 8)
    assert codes[-1][0] == 257
    c["60x50_clear_then_eoi"] = page_file(short, 8, lzw=write_codes(codes[:-1] + [(256, codes[-1][1]), (257, 9)]))
    c["60x50_clear_is_the_last_code"] = page_file(short, 8, lzw=write_codes(codes[:-1] + [(256, codes[-1][1])]))
    for name, blob in c.items():
        _cut[name] = (blob, model_counts(blob))
    return _cut


def test_the_model_confirms_the_cuts():
    c = cut_cases()
    assert MIN == 2048
    assert c["130x120_noise_m8"][1] == [4] and c["200x200_noise_m8"][1] == [11]
    segs = segments_of(streams(c["130x120_noise_m8"][0])[0][1], 8)
    # a full table is 1 + 254 codes of 9 bits, 512 of 10, 1024 of 11, 2048 of 12 and the clear: 43267 bits, 5408 bytes and
    # three bits (the page's own leading clear makes segment 0 nine bits longer)
    full = 9 * 255 + 10 * 512 + 11 * 1024 + 12 * 2048 + 12
    assert [e - s for s, e, _ in segs[:-1]] == [full + 9, full, full] and full // 8 == 5408
    assert c["200x200_noise_never_clear"][1] == [1] and c["200x200_runs_m8"][1][0] > 1
    assert c["200x200_noise_m2"][1] == [3] and c["200x200_noise_m4"][1] == [5]         # the table filled at least twice
    assert c["130x120_noise_m8_interlaced"][1] == [4] and c["131x75_noise_m6_interlaced"][1][0] >= 2
    for name in ("130x120_noise_m8_interlaced", "131x75_noise_m6_interlaced"):          # a segment starts mid-row
        mcs, data = streams(c[name][0])[0]
        w = int(name.split("x")[0])
        for start, _, _ in segments_of(data, mcs)[1:]:
            assert len(G.lzw_decode(data[: (start + 7) // 8], mcs, 1 << 30)) % w
    # clears every ~1.2 KB: neighbours merge under the 2048-byte bound -- every cut segment holds two of them
    mcs, data = streams(c["130x120_noise_m8_clear_every_1000"][0])[0]
    segs = segments_of(data, mcs)
    clears = sum(1 for code, _, _, _ in read_codes(data, mcs) if code == 256)
    assert clears == 16 and len(segs) == 8 and all(MIN * 8 <= e - s < 2 * MIN * 8 for s, e, _ in segs[:-1])
    rounds = sorted(n for n in c if "_of_its_round_" in n)
    assert [n.split("code_")[1].split("_")[0] for n in rounds] == ["0", "0", "1", "63"] and len({n[-2:] for n in rounds}) == 2
    for n in rounds + ["60x50_clear_then_eoi", "60x50_clear_is_the_last_code"]:
        assert c[n][1] == [2], n
    assert c["130x120_two_clears_at_a_cut"][1] == [4]
    mcs, data = streams(c["60x50_clear_is_the_last_code"][0])[0]
    assert segments_of(data, mcs)[-1][0] > len(data) * 8 - 8                            # the last segment is empty


def test_the_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "impgpu.h")).read()
    assert int(re.search(r"#define IMPGPU_GIF_SPLIT_MIN_BYTES (\d+)", text).group(1)) == imp.GIF_SPLIT_MIN_BYTES
    assert int(re.search(r"#define IMPGPU_GIF_SPLIT (\d+)", text).group(1)) == imp.GIF_SPLIT == 1


def test_pages_made_to_be_cut_equal_the_plain_decoder():
    for name, (blob, counts) in cut_cases().items():
        rc, segs = same_as_the_plain_decoder(blob, name, counts)
        assert rc == 0, name
        parsed, _ = G.parse(blob)                          # ... and the writer's own decoder
        assert imp.gif_pages_split(blob)[1] == G.planes(parsed), name


def test_every_written_file_equals_the_plain_decoder():
    for name, (blob, pages) in pin_cases().items():
        rc, segs = same_as_the_plain_decoder(blob, name)
        assert rc == 0 and imp.gif_pages_split(blob)[1] == G.planes(pages), name
    blob, pages = album_file()
    rc, segs = same_as_the_plain_decoder(blob, "album")
    assert rc == 0 and segs == [1] * 6 and imp.gif_pages_split(blob)[1] == G.planes(pages)


def test_both_damage_sets_get_the_plain_decoders_verdicts():
    for name, stream in damaged_streams().items():
        for trailing in (False, True):
            rc, segs = same_as_the_plain_decoder(damaged_file(stream, trailing), name)
            assert rc == imp.IMP_ERROR_DECODE_FAILED and segs == [1] * (1 + trailing), name
    blob, _ = album_file()
    good = G.write([tiny()])
    at = good.index(b"\x2c", 13)
    long_block = bytearray(good)
    long_block[-5] = 200
    container = [blob[:cut] for cut in range(6, len(blob))] + [G.write([tiny()], trailer=False), header_only_size(0, 5), header_only_size(5, 0),
                                                                good[:at] + b"\x99" + good[at + 1:], bytes(long_block)]
    for k, f in enumerate(container):
        assert imp.gif_pages_split(f) == (imp.IMP_ERROR_DECODE_FAILED, None, None) and raw(f, False)[0] == imp.IMP_ERROR_DECODE_FAILED, k
    no_table = G.make_page(np.zeros((2, 2), np.uint8), palette=None, mcs=2)
    assert imp.gif_pages_split(G.write([no_table])) == (imp.IMP_ERROR_UNSUPPORTED, None, None)
    assert imp.lib.impgpu_gif_pages_split(good, len(good), None, 0, None, (C.c_int * 1)(), -1) == imp.IMP_ERROR_INVALID_ARGS


_damage = {}


def damage_behind_a_cut():
    """name -> (file, which verdict the damage earns): a valid 130 x 120 noise page of 4 segments, damaged behind a cut"""
    if _damage:
        return _damage
    idx = noise(130, 120, 8)
    px = idx.reshape(-1)
    data = G.lzw_encode(px, 8)
    segs = segments_of(data, 8)
    assert len(segs) == 4
    codes = read_codes(data, 8)
    _damage["cut short inside segment 2"] = (page_file(idx, 8, lzw=data[: (segs[2][0] + segs[2][1]) // 16]), "short")
    extra = np.concatenate([px, noise(9, 1, 8, 9).reshape(-1)])
    _damage["nine indices too many in the last segment"] = (page_file(idx, 8, lzw=G.lzw_encode(extra, 8)), "long")
    assert len(G.lzw_decode(data[: (segs[1][0] + 7) // 8], 8, 1 << 30)) < 130 * 60 < len(G.lzw_decode(data[: segs[1][1] // 8], 8, 1 << 30))
    _damage["indices beyond the page in a middle segment"] = (page_file(idx[:60], 8, lzw=data), "long")
    k = [i for i, c in enumerate(codes) if c[2] == segs[2][0]][0]                      # the first code behind the second cut
    assert codes[k - 1][0] == 256 and codes[k][0] < 256
    _damage["a non-literal first code behind the second cut"] = (page_file(idx, 8, lzw=write_codes(codes[:k] + [(300, 9)] + codes[k + 1:])), "invalid")
    j = [i for i, c in enumerate(codes) if segs[1][0] < c[2] < segs[1][1] and c[3] == 700][0]    # 700 codes into segment 1: the free code is 957
    assert codes[j][1] == 10
    _damage["a code above the free code in the middle of segment 1"] = (page_file(idx, 8, lzw=write_codes(codes[:j] + [(1000, 10)] + codes[j + 1:])), "invalid")
    return _damage


def test_damage_behind_a_cut_is_found_and_stays_inside_the_planes():
    for name, (blob, kind) in damage_behind_a_cut().items():
        assert imp.gif_info(blob)[0] == 0, name
        mcs, data = streams(blob)[0]
        assert len(segments_of(data, mcs)) >= 2, name
        rc, segs = same_as_the_plain_decoder(blob, name)    # (raw() holds the planes in a guard frame and checks it)
        assert rc == imp.IMP_ERROR_DECODE_FAILED, name
        assert imp.gif_pages(blob, 1)[0] == imp.IMP_ERROR_DECODE_FAILED, name


def test_the_flagless_diagnostic_keeps_its_range():
    good = G.write([tiny()])
    assert imp.lib.impgpu_gif_pages(good, len(good), 2, None, 0, None) == imp.IMP_ERROR_INVALID_ARGS
    n = C.c_size_t(0)
    assert imp.lib.impgpu_gif_pages(good, len(good), 2, None, 0, C.byref(n)) == imp.IMP_ERROR_INVALID_ARGS and n.value == 0
    for how in (0, 1):
        assert imp.gif_pages(good, how)[0] == 0
