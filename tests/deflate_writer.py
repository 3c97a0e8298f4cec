"""A small raw-deflate WRITER for the tests (RFC 1951): streams built from explicit token lists, so that a test can ask for
exactly the match it means -- distance 1 with length 258, distance 32 768, a match straddling a given offset -- which zlib's
own compressor produces only by accident.  Blocks are stored (3.2.4) or fixed-Huffman (3.2.6); any sequence of them.  The
DECODING -- the thing under test -- is never done with this file: tests/test_inflate_lanes.py first pins every stream it
makes against zlib.decompress.

    tokens: ints 0..255 (literals) and (length, distance) pairs, 3 <= length <= 258, 1 <= distance <= 32768
    stream = zlib_wrap(deflate([fixed(tokens), stored(b"..."), fixed(more, final=True)]))
"""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        """`count` bits of `value`, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, count):
        """a Huffman code: most significant bit first (3.1.1)"""
        for i in range(count - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data


def _fixed_ll(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def stored(data, final=False):
    """a stored block (at most 65 535 bytes)"""
    data = bytes(data)
    assert len(data) <= 0xffff
    return ("stored", data, final)


def fixed(tokens, final=False, end=True):
    """a fixed-Huffman block of literals and (length, distance) pairs; end=False leaves out the end-of-block code (a block
    that simply stops: for streams that are cut there)"""
    return ("fixed", list(tokens), final, end)


def deflate(blocks):
    """the raw deflate stream of the blocks, in order"""
    w = BitWriter()
    for b in blocks:
        if b[0] == "stored":
            _, data, final = b
            w.bits(1 if final else 0, 1)
            w.bits(0, 2)
            w.align()
            w.raw(struct.pack("<HH", len(data), len(data) ^ 0xffff) + data)
            continue
        _, tokens, final, end = b
        w.bits(1 if final else 0, 1)
        w.bits(1, 2)
        for t in tokens:
            if isinstance(t, int):
                _fixed_ll(w, t)
                continue
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= 32768
            c = max(i for i in range(29) if LEN_BASE[i] <= length) if length < 258 else 28
            _fixed_ll(w, 257 + c)
            w.bits(length - LEN_BASE[c], LEN_EXTRA[c])
            d = max(i for i in range(30) if DIST_BASE[i] <= dist)
            w.code(d, 5)
            w.bits(dist - DIST_BASE[d], DIST_EXTRA[d])
        if end:
            _fixed_ll(w, 256)
    w.align()
    return bytes(w.out)


def expand(blocks):
    """the bytes the blocks MEAN (the writer's own model, checked against zlib by the tests)"""
    out = bytearray()
    for b in blocks:
        if b[0] == "stored":
            out += b[1]
            continue
        for t in b[1]:
            if isinstance(t, int):
                out.append(t)
            else:
                length, dist = t
                assert dist <= len(out)
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out)


def zlib_wrap(raw, data=b""):
    """RFC 1950: CMF/FLG of a 32 KB window in front, the Adler-32 of `data` behind"""
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data) & 0xffffffff)


def gray_png(stream, width, height=1):
    """the stream as the IDAT of an 8-bit gray PNG of width x height (its scanlines are whatever the stream inflates to)"""
    from png_writer import chunk

    ihdr = struct.pack(">IIBBBBB", width, height, 8, 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")
