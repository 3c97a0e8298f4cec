"""impgpu_png_inflate_lanes (host, no device): the rounds of k_png_inflate (csrc/imp_inflate_lanes.h), one lane after the
other.  Every case compares its verdict and bytes with zlib.decompressobj().decompress(z, out_size) and with the library's
host route -- impgpu_png_scanlines (imp::inflate_exact) on an 8-bit gray PNG wrapped round the stream, which also fails on a
filter byte above 4, so the comparison allows for exactly that.  tests/deflate_writer.py's streams are pinned against
zlib.decompress first."""
import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_writer as D
import inflate_cases as K
import ngx_http_imgproc_amd as imp

OK, DAMAGED, SHORT = 0, 1, 2


def zlib_says(z, n):
    """(ok, bytes): zlib's verdict on `n` bytes wanted from z.  ok is None where zlib fails on n bytes but delivers n - 1:
    zlib decodes -- and judges -- one symbol, or one block header, past a full output before it looks at the room left, so
    its complaint there may be about the byte at n - 1 or about what follows it.  inflate_exact, the lanes and libpng's
    reading of an image do not look behind a full output; the host route decides such a case."""
    try:
        got = zlib.decompressobj().decompress(z, n) if n else b""
    except zlib.error:
        if n > 1:
            try:
                got = zlib.decompressobj().decompress(z, n - 1)
                if len(got) == n - 1:
                    return None, got
            except zlib.error:
                pass
        return False, None
    return len(got) == n, got


def host_route(z, n, shape=None):
    """impgpu_png_scanlines on the gray PNG whose scanlines are n bytes -> (code, bytes), or None where no such PNG exists"""
    shape = shape or K.shape_for(n)
    if shape is None:
        return None
    w, h = shape
    assert (w + 1) * h == n
    blob = D.gray_png(z, w, h)
    buf = np.zeros(n, np.uint8)
    length = C.c_size_t()
    rc = imp.lib.impgpu_png_scanlines(blob, len(blob), buf.ctypes.data, n, C.byref(length))
    assert length.value == n
    return rc, buf.tobytes(), w + 1


def check(z, n, want=None, status=None, zlib_too=True, shape=None):
    rc, st, got = imp.png_inflate_lanes(z, n)
    assert (rc == 0) == (st == OK) and rc in (0, imp.IMP_ERROR_DECODE_FAILED)
    if status is not None:
        assert st == status, (st, status)
    if want is not None:
        assert rc == 0 and got == want[:n]
    host = host_route(z, n, shape)
    if host is not None:
        hrc, hgot, stride = host
        filter_bad = rc == 0 and any(got[at] > 4 for at in range(0, n, stride))
        assert (hrc == 0) == (rc == 0 and not filter_bad), (hrc, rc, st, filter_bad)
        if hrc == 0:
            assert hgot == got
    if zlib_too:
        zok, zgot = zlib_says(z, n)
        if zok is None:
            assert host is not None                          # (decided by the host route above)
            if rc == 0:
                assert got[:n - 1] == zgot
        else:
            assert (rc == 0) == zok, (rc, st, zok, n, len(z))
            if zok:
                assert got == zgot
    return st


# ---------------------------------------------------------------- the writer, pinned
def test_the_stream_writer_means_what_zlib_reads():
    rng = np.random.default_rng(3)
    lit = [int(v) for v in rng.integers(0, 256, size=300)]
    cases = [
        [D.fixed(lit, final=True)],
        [D.stored(bytes(lit)), D.fixed(lit[:5] + [(258, 1), (3, 5), (17, 300), (130, 2)], final=True)],
        [D.fixed([1, 2, 3, (3, 3), (6, 6), (5, 2)]), D.stored(b""), D.stored(b"xyz"), D.fixed([(3, 3), 9], final=True)],
        [D.fixed([0] + [(l, 1) for l in range(3, 259)], final=True)],
        [D.stored(bytes(rng.integers(0, 256, size=40000, dtype=np.uint8))), D.fixed([(258, 32768), (3, 32768), (200, 24577), (9, 24576)], final=True)],
    ]
    for blocks in cases:
        data = D.expand(blocks)
        assert zlib.decompress(D.deflate(blocks), -15) == data
        assert zlib.decompress(D.zlib_wrap(D.deflate(blocks), data)) == data
    z, data = K.far_stream()
    assert zlib.decompress(z) == data and len(data) == 40258


# ---------------------------------------------------------------- zlib's own output
SIZES = [1, 2, 7, 300, 4098, 33000, 70000]
STRATEGIES = [("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman", zlib.Z_HUFFMAN_ONLY),
              ("filtered", zlib.Z_FILTERED)]


@pytest.mark.parametrize("kind", ["photo", "solid", "random", "skewed", "steep"])
def test_zlibs_own_streams(kind):
    for n in SIZES:
        shape = K.shape_for(n)
        data = K.rows_of(K.content(kind, n, n), shape[0] + 1 if shape else n)
        for level in (0, 1, 6, 9):
            assert check(zlib.compress(data, level), n, want=data) == OK
        for _, strategy in STRATEGIES[1:]:
            assert check(K.compress(data, 6, strategy), n, want=data) == OK


def test_level_0_makes_two_stored_blocks():
    n = 67340
    data = K.rows_of(K.content("random", n), 3367)
    z = zlib.compress(data, 0)
    assert len(z) == 2 + n + 2 * 5 + 4                      # two stored blocks: 65 535 + the rest
    check(z, n, want=data, status=OK)
    check(z, n - 1000, want=data, status=OK)                 # complete inside the second block
    check(z, 65535, want=data, status=OK)                    # complete at the first block's last byte


def test_sync_flushes_leave_many_blocks_and_empty_stored_ones():
    n = 70000
    data = K.rows_of(K.content("photo", n, 4), 3500)
    z = K.compress(data, 6, sync_every=1000)
    assert z.count(b"\x00\x00\xff\xff") >= 69
    check(z, n, want=data, status=OK)
    z = K.compress(data, 6, zlib.Z_FIXED, sync_every=1000)
    check(z, n, want=data, status=OK)


def test_the_longest_codes():
    """the steep histogram under Z_HUFFMAN_ONLY: literal codes of 15 bits (zlib's length limit is reached)"""
    n = 70000
    data = K.rows_of(K.steep(n), 3500)
    z = K.compress(data, 6, zlib.Z_HUFFMAN_ONLY)
    check(z, n, want=data, status=OK)
    check(z[:-5], n, status=OK)                              # (the end-of-block code is not needed: the output is full before it)
    check(z[:-30], n, status=SHORT)


# ---------------------------------------------------------------- hand-made token lists
def wrapped(blocks):
    data = D.expand(blocks)
    return D.zlib_wrap(D.deflate(blocks), data), data


def test_distance_1_length_258_and_every_short_overlap():
    z, data = wrapped([D.fixed([0, (258, 1)], final=True)])
    check(z, len(data), want=data, status=OK)
    for dist in range(1, 9):
        for length in (3, max(3, dist + 1), 64, 65, 258):
            z, data = wrapped([D.fixed([0] + list(range(1, dist)) + [(length, dist), 9, (2 * dist + 3, dist + 1)], final=True)])
            check(z, len(data), want=data, status=OK)


def test_distance_32768_before_and_behind_the_rings_wrap():
    for n in (32768, 40000, 32768 + 8192, 90000):
        z, data = K.far_stream(n)
        check(z, len(data), want=data, status=OK)
    z, data = K.far_stream(40000, 200, 201)                  # (a 200 x 200 gray image: the host route sees this one too)
    check(z, len(data), want=data, status=OK, shape=(200, 200))
    # one byte farther than the output reaches: damaged
    blocks = [D.stored(bytes(20000)), D.stored(bytes(12767)), D.fixed([(3, 32768)], final=True)]
    check(D.zlib_wrap(D.deflate(blocks)), 32770, status=DAMAGED)
    blocks = [D.fixed([0, 1, (3, 3)], final=True)]
    check(D.zlib_wrap(D.deflate(blocks)), 5, status=DAMAGED)


def test_a_match_whose_source_is_the_token_before_it():
    z, data = wrapped([D.fixed([1, 2, 3, (3, 3), (6, 6), (5, 2), (12, 12), 4, (3, 1), (4, 4)], final=True)])
    check(z, len(data), want=data, status=OK)


def test_matches_that_straddle_a_rounds_end():
    """a round holds 512 tokens and stops before a token that would start past byte 7934 of it: matches at those edges"""
    lit = [0] + [int(v) for v in np.random.default_rng(8).integers(0, 256, size=600)]
    for k in (509, 510, 511, 512, 513):                      # the match is token k: the last of a round, the first of the next
        z, data = wrapped([D.fixed(lit[:k] + [(258, 200), (40, 258), 5, (30, 1)] + lit[:20], final=True)])
        check(z, len(data), want=data, status=OK)
    for first in (7930, 7934, 7935, 8191, 8192):             # a match of 258 from that byte of the round on
        runs = [0] + [(258, 1)] * (first // 258)
        fill = first - 1 - 258 * (first // 258)
        tokens = runs + [3] * fill + [(258, 1000), 8, (258, 258), (100, 3)]
        z, data = wrapped([D.fixed(tokens, final=True)])
        assert len(data) == first + 258 + 1 + 258 + 100
        check(z, len(data), want=data, status=OK)


def test_a_match_that_straddles_out_size():
    z, data = wrapped([D.fixed([0, 1, 2, 3, 4, (100, 5), (50, 2), 7], final=True)])
    for n in (6, 50, 104, 105, 106, 154, 155):
        check(z, n, want=data, status=OK)


def test_garbage_behind_a_full_output_is_not_read():
    lit = [0] + list(range(1, 60))
    garbage = bytes([0xff, 0xfe, 0x07, 0xff]) * 16
    # in the same block: the block never ends, what follows is no code at all
    z = b"\x78\x9c" + D.deflate([D.fixed(lit + [(40, 7)], end=False)]) + garbage
    # (zlib itself decodes -- and judges -- one symbol, or one block header, past a full output before it looks at the room
    # left; inflate_exact and the lanes do not, and libpng shows such a file's tail only as a benign warning: not compared)
    check(z, 100, want=D.expand([D.fixed(lit + [(40, 7)])]), status=OK, zlib_too=False)
    check(z, 101, zlib_too=False)                            # (one byte more: whatever the garbage means, nobody accepts it ...)
    assert imp.png_inflate_lanes(z, 400)[0] != 0             # (... or 300 bytes more)
    # in a later block: block type 3 behind a complete, non-final block
    z = b"\x78\x9c" + D.deflate([D.fixed(lit)]) + b"\x07" + garbage
    check(z, 60, want=bytes(lit), status=OK, zlib_too=False)
    check(z, 61, status=DAMAGED)
    # behind the final block
    z, data = wrapped([D.fixed(lit, final=True)])
    check(z + garbage, 60, want=data, status=OK)


def test_a_final_block_that_ends_one_byte_short():
    z, data = wrapped([D.fixed([0] + list(range(1, 60)), final=True)])
    check(z, len(data) + 1, status=SHORT)
    z, data = wrapped([D.stored(bytes(60), final=True)])
    check(z, len(data) + 1, status=SHORT)
    z = zlib.compress(K.rows_of(K.content("photo", 5000), 5000), 6)
    check(z, 5001, status=SHORT)


# ---------------------------------------------------------------- damage
def test_every_truncation_of_two_small_streams():
    a = K.rows_of(K.content("skewed", 400), 400)
    for z, data in ((zlib.compress(a, 6), a), wrapped([D.stored(b"\x00abc"), D.fixed([1, 2, 3, (30, 2)]), D.stored(b"tail" * 9, final=True)])):
        for cut in range(len(z) + 1):
            st = check(z[:cut], len(data))
            if cut >= len(z) - 4:
                assert st == OK                              # (the Adler-32 trailer is not looked at)
            elif cut <= len(z) - 8:                          # (in between lies the end-of-block code, which a full output does not need)
                assert st == SHORT


def test_every_single_bit_flip_of_a_dynamic_stream():
    rng = np.random.default_rng(12)
    data = K.rows_of(bytes(int(v) for v in np.minimum(rng.geometric(0.25, size=360), 30)), 360)
    z = zlib.compress(data, 6)
    assert 180 <= len(z) <= 220 and (z[2] >> 1) & 3 == 2      # about 200 bytes, a dynamic block
    verdicts = {OK: 0, DAMAGED: 0, SHORT: 0}
    for bit in range(len(z) * 8):
        b = bytearray(z)
        b[bit >> 3] ^= 1 << (bit & 7)
        verdicts[check(bytes(b), len(data))] += 1
    assert verdicts[OK] >= 32 and verdicts[DAMAGED] > 100 and verdicts[SHORT] > 100, verdicts


def test_the_header_cases():
    data = K.rows_of(K.content("photo", 300), 300)
    z = zlib.compress(data, 6)
    for cmf, flg in ((0x79, 0x9c), (0x88, 0x1c), (0x78, 0x9d), (0x78, 0xbb), (0x77, 0x9c)):   # method 9, window 64 K, FCHECK, FDICT, method 7
        check(bytes([cmf, flg]) + z[2:], len(data), status=DAMAGED)
    for cmf, flg in ((0x78, 0x01), (0x78, 0x5e), (0x78, 0xda), (0x08, 0x1d), (0x68, 0x81)):   # other levels, smaller windows: fine
        check(bytes([cmf, flg]) + z[2:], len(data), want=data, status=OK)
    check(b"", 10, status=SHORT, zlib_too=False)
    check(b"\x78", 10, status=SHORT)
    check(b"\x78\x9c", 10, status=SHORT)
    check(b"\x78\x9c" + b"\x07", 10, status=DAMAGED)                               # block type 3
    check(b"\x78\x9c" + b"\x01\x05\x00\xfa\xfe" + b"hello", 5, status=DAMAGED)      # LEN != ~NLEN
    check(b"\x78\x9c" + b"\x01\x05\x00\xfa\xff" + b"\x00ello", 5, want=b"\x00ello", status=OK)
    check(b"\x78\x9c" + b"\x01\x05\x00\xfa\xff" + b"\x00ell", 5, status=SHORT)
    # dynamic headers: HLIT = 287, HDIST = 31, a repeat code with no previous length, a repeat past HLIT + HDIST
    def dynamic(hlit, hdist, hclen, rest):
        w = D.BitWriter()
        w.bits(1, 1); w.bits(2, 2); w.bits(hlit - 257, 5); w.bits(hdist - 1, 5); w.bits(hclen - 4, 4)
        for value, count in rest:
            w.bits(value, count)
        w.align()
        return b"\x78\x9c" + bytes(w.out) + bytes(16)
    check(dynamic(287, 1, 4, []), 10, status=DAMAGED)
    check(dynamic(257, 31, 4, []), 10, status=DAMAGED)
    cl = [(1, 3), (0, 3), (0, 3), (1, 3)]                     # 16 and 0 one bit each: 0 is code 0, 16 is code 1
    check(dynamic(257, 1, 4, cl + [(1, 1), (0, 2)]), 10, status=DAMAGED)            # 16 first: nothing to repeat
    cl = [(0, 3), (0, 3), (1, 3), (1, 3)]                     # 18 and 0 one bit each: 0 is code 0, 18 is code 1
    check(dynamic(257, 1, 4, cl + [(1, 1), (127, 7), (1, 1), (127, 7)]), 10, status=DAMAGED)     # 138 + 138 zeros > 258
    check(dynamic(257, 1, 4, [(0, 3)] * 4), 10, status=DAMAGED)                     # no code-length code at all
    check(dynamic(257, 1, 4, [(0, 3), (0, 3), (0, 3), (1, 3)]), 10, status=DAMAGED)  # an incomplete one
    w = D.BitWriter()
    w.bits(1, 1); w.bits(1, 2); D._fixed_ll(w, 0); D._fixed_ll(w, 286); w.align()
    check(b"\x78\x9c" + bytes(w.out) + bytes(8), 10, status=DAMAGED)
    w = D.BitWriter()
    w.bits(1, 1); w.bits(1, 2); D._fixed_ll(w, 0); D._fixed_ll(w, 257); w.code(30, 5); w.align()
    check(b"\x78\x9c" + bytes(w.out) + bytes(8), 10, status=DAMAGED)


def test_a_guarded_destination():
    """canaries on both sides of the output, for sound and for damaged streams"""
    z, data = K.far_stream(40000)
    streams = [z, z[:len(z) // 2], z[:20000] + bytes([z[20000] ^ 0x10]) + z[20001:], zlib.compress(K.content("photo", 9000), 6)]
    for s in streams:
        for n in (1, 100, 9000, len(data), len(data) + 300):
            buf = np.full(n + 128, 0xA5, np.uint8)
            st = C.c_int(-1)
            imp.lib.impgpu_png_inflate_lanes(s, len(s), buf.ctypes.data + 64, n, C.byref(st))
            assert (buf[:64] == 0xA5).all() and (buf[64 + n:] == 0xA5).all(), (n, st.value)


def test_the_arguments():
    st = C.c_int(-1)
    assert imp.lib.impgpu_png_inflate_lanes(None, 5, None, 0, C.byref(st)) == imp.IMP_ERROR_INVALID_ARGS
    assert imp.lib.impgpu_png_inflate_lanes(b"\x78\x9c\x03\x00", 4, None, 0, None) == 0
    assert imp.PNG_DEVICE_INFLATE == 8 and not (imp.PNG_ALL & imp.PNG_DEVICE_INFLATE)
    # impgpu_png_info_ex and impgpu_png_scanlines_ex ignore the bit
    blob = D.gray_png(zlib.compress(bytes(8)), 3, 2)
    assert imp.png_info_ex(blob, imp.PNG_DEVICE_INFLATE) == imp.png_info_ex(blob, 0)
    assert imp.png_scanlines_ex(blob, imp.PNG_DEVICE_INFLATE | imp.PNG_ALL) == imp.png_scanlines_ex(blob, imp.PNG_ALL)
