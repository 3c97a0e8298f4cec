"""Hand-written lossless WebP (VP8L) streams for the decoder's tests: what an encoder does not emit at small sizes.  A
file is written from TOKENS -- ("lit", argb), ("copy", length, distance code) and ("cache", argb) -- by a writer that
knows the format from include/impgpu.h and webp_writer / webp_lz_writer (container, prefix codes, the prefix coding of
lengths and distances, _pack) and nothing of the library.  Pillow's libwebp is the judge of every file: the expected
frames of tests/golden/webp_dec come from its decoder, never from this module's idea of the pixels.

    cases()      [(name, file bytes)] in a fixed order: everything is seeded
"""
import numpy as np

import webp_lz_writer as LZ
import webp_writer as W

# VP8L's distance map, codes 1..120, as (xi, yi): the distance is xi + yi * width (below 1: 1).  The specification's list;
# the per-code files below put every entry before Pillow's decoder.
DISTANCE_MAP = (
    (0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3), (3, 1), (-3, 1),
    (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4), (4, 2), (-4, 2), (0, 5), (3, 4),
    (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2), (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3),
    (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2), (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3),
    (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1), (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7),
    (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5), (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7),
    (7, 5), (-7, 5), (8, 4), (6, 7), (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7))
assert len(DISTANCE_MAP) == 120 and len(set(DISTANCE_MAP)) == 120


def code_distance(code, width):
    """a distance code -> pixels"""
    if code > 120:
        return code - 120
    xi, yi = DISTANCE_MAP[code - 1]
    return max(1, xi + yi * width)


def cache_hash(argb, bits):
    return ((argb * 0x1E35A7BD) & 0xFFFFFFFF) >> (32 - bits)


class Bits:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, v, n):
        if n:
            self.vals.append(int(v))
            self.lens.append(int(n))

    def pairs(self, pairs):
        for v, n in pairs:
            self.put(v, n)

    def payload(self):
        return W._pack(self.vals, self.lens)[0]


def simple_code(symbols, alphabet):
    """the simple form for one or two symbols (< 256) -> (header bits, lengths, codes)"""
    symbols = sorted(symbols)
    lengths, codes = [0] * alphabet, [0] * alphabet
    first8 = int(symbols[0] > 1)
    bits = [(1, 1), (len(symbols) - 1, 1), (first8, 1), (symbols[0], 8 if first8 else 1)]
    if len(symbols) == 2:
        bits.append((symbols[1], 8))
        lengths[symbols[0]] = lengths[symbols[1]] = 1
        codes[symbols[1]] = 1                     # canonical: the lower symbol is 0
    return bits, lengths, codes


def make_code(hist, alphabet, simple=False):
    used = [n for n, v in enumerate(hist) if v]
    if not used:
        return simple_code([0], alphabet)
    if simple and len(used) <= 2 and max(used) < 256:
        return simple_code(used, alphabet)
    return W.prefix_code(list(hist) + [0] * (alphabet - len(hist)), alphabet)


def token_symbols(tok, cache_bits):
    """a token -> [(which code 0..4, symbol, extra value, extra bits)]"""
    if tok[0] == "lit":
        v = tok[1]
        return [(0, (v >> 8) & 255, 0, 0), (1, (v >> 16) & 255, 0, 0), (2, v & 255, 0, 0), (3, v >> 24, 0, 0)]
    if tok[0] == "cache":
        return [(0, 280 + cache_hash(tok[1], cache_bits), 0, 0)]
    ls, lv, ln = LZ.prefix_value(tok[1])
    ds, dv, dn = LZ.prefix_value(tok[2])
    return [(0, 256 + ls, lv, ln), (4, ds, dv, dn)]


def token_step(tok):
    return tok[1] if tok[0] == "copy" else 1


def image_stream(out, tokens, width, cache_bits=0, meta=None, simple=False, is_main=True):
    """an entropy-coded image: cache size, [meta prefix image], the groups' codes, the tokens.  meta: (bits, HxW groups)"""
    out.put(1 if cache_bits else 0, 1)
    if cache_bits:
        out.put(cache_bits, 4)
    ngroups = 1
    if is_main:
        out.put(1 if meta else 0, 1)
        if meta:
            mbits, groups = meta
            out.put(mbits - 2, 3)
            image_stream(out, [("lit", 0xFF000000 | int(g) << 8) for g in groups.reshape(-1)], groups.shape[1], is_main=False)
            ngroups = int(groups.max()) + 1
    alphabets = (280 + ((1 << cache_bits) if cache_bits else 0), 256, 256, 256, 40)
    group_of, pos = [], 0
    for tok in tokens:
        group_of.append(int(meta[1][(pos // width) >> meta[0], (pos % width) >> meta[0]]) if meta and is_main else 0)
        pos += token_step(tok)
    hists = [[np.zeros(a, np.int64) for a in alphabets] for _ in range(ngroups)]
    for tok, g in zip(tokens, group_of):
        for k, s, _, _ in token_symbols(tok, cache_bits):
            hists[g][k][s] += 1
    codes = []
    for g in range(ngroups):
        codes.append([])
        for k, a in enumerate(alphabets):
            bits, lengths, cds = make_code(hists[g][k], a, simple)
            out.pairs(bits)
            codes[g].append((lengths, cds))
    for tok, g in zip(tokens, group_of):
        for k, s, xv, xn in token_symbols(tok, cache_bits):
            out.put(codes[g][k][1][s], codes[g][k][0][s])
            out.put(xv, xn)


def vp8l(width, height, tokens, transforms=(), alpha=0, **kw):
    """the file.  transforms: ("green",), ("predictor", bits, modes HxW), ("color", bits, elements HxW uint32),
    ("index", [argb ...]) in the order they are written"""
    out = Bits()
    out.pairs([(0x2F, 8), (width - 1, 14), (height - 1, 14), (alpha, 1), (0, 3)])
    for t in transforms:
        out.put(1, 1)
        if t[0] == "green":
            out.put(2, 2)
        elif t[0] in ("predictor", "color"):
            out.put(0 if t[0] == "predictor" else 1, 2)
            out.put(t[1] - 2, 3)
            data = np.asarray(t[2])
            vals = [0xFF000000 | int(v) << 8 for v in data.reshape(-1)] if t[0] == "predictor" else [0xFF000000 | int(v) for v in data.reshape(-1)]
            image_stream(out, [("lit", v) for v in vals], data.shape[1], is_main=False)
        else:
            pal = [int(v) for v in t[1]]
            out.put(3, 2)
            out.put(len(pal) - 1, 8)
            deltas = [pal[0]] + [sum((((pal[i] >> s) - (pal[i - 1] >> s)) & 255) << s for s in (0, 8, 16, 24)) for i in range(1, len(pal))]
            image_stream(out, [("lit", v) for v in deltas], len(pal), is_main=False)
    out.put(0, 1)
    image_stream(out, tokens, width, **kw)
    return W.container(out.payload())


def distinct_pixels(n, seed):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.choice(1 << 24, n, replace=False) + 0xFF000000]


def reference_file(code, width, height, col, row, seed=5):
    """distinct literal pixels and ONE length-1 reference with distance code `code` at (col, row)"""
    px = [0xFF000000 | (i >> 8) << 16 | (i & 255) << 8 | ((i * 5 + seed) & 255) for i in range(width * height)]      # distinct, and small to store
    at = row * width + col
    tokens = [("lit", v) for v in px[:at]] + [("copy", 1, code)] + [("lit", v) for v in px[at + 1:]]
    return vp8l(width, height, tokens)


def cache_file(cache_bits, seed):
    """literals, a copy of earlier pixels, then cache hits on the COPIED colours, a literal, and hits again"""
    width, height = 24, 8
    rng = np.random.default_rng(seed)
    colours = distinct_pixels(40, seed)
    tokens, px, cache = [], [], {}

    def lit(v):
        tokens.append(("lit", v)); px.append(v); cache[cache_hash(v, cache_bits)] = v

    def copy(length, dist):
        tokens.append(("copy", length, dist + 120))
        for _ in range(length):
            v = px[len(px) - dist]
            px.append(v); cache[cache_hash(v, cache_bits)] = v

    def hit(v):
        if cache.get(cache_hash(v, cache_bits)) == v:
            tokens.append(("cache", v)); px.append(v)
        else:
            lit(v)

    for v in colours[:20]:
        lit(v)
    while len(px) < width * height:
        left = width * height - len(px)
        kind = int(rng.integers(0, 4))
        if kind == 0 and left > 12:
            copy(int(rng.integers(2, 12)), int(rng.integers(1, min(len(px), 30))))
            for _ in range(min(3, width * height - len(px))):
                hit(px[len(px) - int(rng.integers(1, 6))])           # a colour the copy (or what lies just before) produced
        elif kind == 1:
            lit(colours[int(rng.integers(0, 40))])
        else:
            hit(px[int(rng.integers(0, len(px)))])
    assert len(px) == width * height and any(t[0] == "cache" for t in tokens)
    return vp8l(width, height, tokens, cache_bits=cache_bits)


def cases():
    out = []
    rng = np.random.default_rng(11)
    # every predictor mode, forced on every tile of a 37 x 21 frame
    y, x = np.mgrid[0:21, 0:37]
    frame = np.clip(np.stack([(x * 5 + y * 3) % 256, (x * 2 + y * 7) % 256, (x + y * 4) % 256], -1) + rng.integers(-9, 10, (21, 37, 3)), 0, 255).astype(np.uint8)
    tx, ty = W.tiles_of(37, 21)
    for mode in range(14):
        out.append(("mode%02d" % mode, W.write(frame, forced_modes=np.full((ty, tx), mode, np.uint8))))
    # every distance code: one length-1 reference at column 16 of row 9 of a 32 x 24 frame of distinct pixels
    for code in list(range(1, 121)) + [121, 300]:
        out.append(("dist%03d" % code, reference_file(code, 32, 24, 16, 9)))
    # mapped distances below 1: a frame 3 wide (no narrower-than-8 entry of the map falls below 1 at 32 wide), the
    # reference at column 0 of row 9
    for code in (18, 28, 44, 60, 64, 80, 88):
        xi, yi = DISTANCE_MAP[code - 1]
        assert xi + yi * 3 < 1
        out.append(("clamp%03d" % code, reference_file(code, 3, 24, 0, 9, seed=6)))
    for bits, seed in ((1, 21), (4, 22), (11, 23)):
        out.append(("cache%02d" % bits, cache_file(bits, seed)))
    # four groups at tile bits 2, each with its own five codes
    w, h = 19, 13
    groups = rng.integers(0, 4, ((h + 3) // 4, (w + 3) // 4))
    groups.reshape(-1)[:4] = (0, 1, 2, 3)
    px = [int(v) | 0xFF000000 for v in rng.integers(0, 1 << 24, w * h)]
    tokens = [("lit", v) for v in px[:60]] + [("copy", 7, 2)] + [("lit", v) for v in px[67:]]
    out.append(("groups4", vp8l(w, h, tokens, meta=(2, groups))))
    # a colour transform with elements of both signs
    w, h = 21, 11
    elems = rng.integers(0, 1 << 24, ((h + 3) // 4, (w + 3) // 4)).astype(np.uint32)
    elems.reshape(-1)[0] = 0x13E020                                   # green->red +0x20, green->blue -0x20, red->blue +0x13
    elems.reshape(-1)[1] = 0xF07F81
    out.append(("colour", vp8l(w, h, [("lit", int(v) | 0xFF000000) for v in rng.integers(0, 1 << 24, w * h)], transforms=(("color", 2, elems),))))
    # palette files whose pixels hold an index past the palette: 5 colours two to a value, 20 colours one to a value
    pal5, pal20 = distinct_pixels(5, 31), distinct_pixels(20, 32)
    w, h = 9, 6
    idx = rng.integers(0, 16, (h, w))
    packed = idx[:, 0::2].copy()
    packed[:, : w // 2] |= idx[:, 1::2] << 4
    out.append(("index_past5", vp8l(w, h, [("lit", 0xFF000000 | int(v) << 8) for v in packed.reshape(-1)], transforms=(("index", pal5),))))
    idx = rng.integers(0, 256, (h, w))
    out.append(("index_past20", vp8l(w, h, [("lit", 0xFF000000 | int(v) << 8) for v in idx.reshape(-1)], transforms=(("index", pal20),))))
    # simple codes of one and of two symbols
    two = [0xFF000000 | (200 if b else 3) << 8 | (1 if c else 0) << 16 | 77 for b, c in rng.integers(0, 2, (15 * 10, 2))]
    out.append(("simple2", vp8l(15, 10, [("lit", v) for v in two], simple=True)))
    out.append(("simple1", vp8l(6, 5, [("lit", 0xFF102030)] * 30, simple=True)))
    # the transforms in an order libwebp's encoder does not use: colour transform, predictor, subtract-green; and colour
    # indexing LAST, behind subtract-green and the predictor
    w, h = 18, 9
    modes = rng.integers(0, 14, ((h + 3) // 4, (w + 3) // 4))
    elems = rng.integers(0, 1 << 24, ((h + 3) // 4, (w + 3) // 4)).astype(np.uint32)
    lits = [("lit", int(v) | 0xFF000000) for v in rng.integers(0, 1 << 24, w * h)]
    out.append(("order_cpg", vp8l(w, h, lits, transforms=(("color", 2, elems), ("predictor", 2, modes), ("green",)))))
    idx = rng.integers(0, 4, (h, (w + 3) // 4 * 4))
    packed = idx[:, 0::4] | idx[:, 1::4] << 2 | idx[:, 2::4] << 4 | idx[:, 3::4] << 6
    out.append(("order_gpi", vp8l(w, h, [("lit", 0xFF000000 | int(v) << 8) for v in packed.reshape(-1)],
                                  transforms=(("green",), ("predictor", 2, modes), ("index", distinct_pixels(4, 33))))))
    return out
